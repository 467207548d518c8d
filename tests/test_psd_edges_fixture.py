"""tests/golden/psd_edges.npz (tests/golden/make_psd_edges.py; read by tests/test_gpu_psd_edges.py on the
GPU) checked on the CPU without mpmath: every case's eigenvalues keep clear of ε and 10 ε by more than
1e3 d 2^-52 max|λ| (the clamp set and the near-null count are decided), and numpy.linalg.eigh meets every
bar of the GPU test against the stored 60-digit values, with margin: the bars ask nothing of the kernels
that a plain f64 eigh does not deliver a hundred times over."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def test_fixture_is_decided_and_eigh_meets_the_bars_with_margin():
    import make_psd_edges as P
    assert os.path.getsize(P.NPZ) < 1 << 20
    n, worst = P.check()
    assert n == len(P.families()) and worst < 1e-2, (n, worst)


def test_fixture_holds_the_families_matrices():
    """The stored matrices are the generator's (structure exact: zeros, diagonals, 1e-160 couplings; the
    rest to the rounding of a QR on another BLAS), and the stated spectra are what mpmath found."""
    import make_psd_edges as P
    cs = {c["name"]: c for d in P.SIZES for c in P.load()[d]}
    fam = P.families()
    assert list(cs) and set(cs) == {n for n, _ in fam}
    for name, M in fam:
        S = cs[name]["M"]
        assert S.shape == M.shape and np.array_equal(S == 0.0, M == 0.0), name
        assert np.max(np.abs(S - M)) <= 1e-12 * max(np.max(np.abs(M)), 1e-300), name
    lam = cs["d_tiny_active_d22"]["lam"]
    np.testing.assert_allclose(lam[:3], [-3e-12, 0.5e-12, 9e-12], rtol=1e-6)
    np.testing.assert_allclose(cs["d_tiny_active_d22"]["cert"][[0, 5]], [np.hypot(0.5e-12, 4e-12), 3.0], rtol=1e-9)
    np.testing.assert_allclose(cs["c_tiny_inactive_d22"]["cert"][[0, 5]], [0.0, 3.0])
    np.testing.assert_allclose(cs["e_zero_d22"]["cert"], [np.sqrt(22.0) * 1e-12, 0, 1e-12, 1e-12, 1, 22], rtol=1e-15)
    np.testing.assert_allclose(cs["b_clusters_d22"]["lam"], [1e-5] * 11 + [1e5] * 11, rtol=1e-9, atol=1e-9)
    K = cs["h_skew_d22"]["M"]
    np.testing.assert_allclose(cs["h_skew_d22"]["cert"][1], np.linalg.norm(0.5 * (K - K.T)), rtol=1e-14)
    assert np.max(np.abs(cs["g_negdef_d22"]["Mp"] - 1e-12 * np.eye(22))) < 1e-27
    assert np.count_nonzero(np.abs(cs["i_blocks_1e-160_d22"]["M"]) < 1e-150) == 2 * 121
