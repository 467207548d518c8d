"""The PSD projection and its ConditioningCert at the edges of the spectrum: ill-conditioned, repeated,
tiny (around ε = 1e-12 and the near-null threshold 10 ε), exactly diagonal / block-diagonal, rank-deficient,
negative definite, non-symmetric and 1e-160-coupled inputs (tests/golden/psd_edges.npz, families a-i of
tests/golden/make_psd_edges.py), against eigenvalues and the clamped reconstruction computed at 60 digits.

Entries (one batched launch over all cases of a size):
  * domain_projection_psd_batch at d = 22 (parallel Jacobi), 6, 3 (psd_project3) and 23 (padded path);
  * info_fusion_additive_batch with L_ev = 0, alpha = 0, and hypothesis_barycenter_projection with one
    hypothesis of weight 1: the operand is exactly M, projected by wg_psd_project_certified (Cholesky
    shortcut + Householder / Sturm ConditioningCert of gc_cond.h, or the Jacobi path when a clamp is active);

Left out: the in-scan certificates (gc_certs.hip k_hyp_certs) of an H = 3 scan whose priors' L are three
family-a matrices. The scan is not well-posed in the oracle: a 1-ulp change of the entries of the prior L
(cond 1e8 / 1e10 / 1e12, λ_max = 1e4) moves the oracle's own Σ and dΨ_proc by 18 / 58 / 76 times their
1e-8 bars, T by up to 970 times its bar and the predict eig_max by 1e-9 / 3e-7 / 2e-5 relative (two f64
inversions of L in predict_diffusion); the device differed from the oracle by just those amounts (eig_max
2e-7 / 2e-5 relative). Scaled into the identity prior's 1e-6 range it is worse (1e6 .. 1e8 bars). The
same kernel code (wave_conditioning) is covered above through wg_psd_project_certified, and the in-scan
launch by test_gpu_degenerate_scans.test_first_scan_on_empty_map_with_inscan_certs.

Bars (make_psd_edges.bars, the project's own of _cond_fields / _cert6, here against the mp values; numpy's
eigh meets each with > 100x margin, tests/test_psd_edges_fixture.py): eig_max 1e-10 relative, eig_min
1e-12 eig_max absolute, near-null count exact, M_psd 1e-12 max(|M|, |M_psd|) max(1, d / 16) absolute, both
deltas 1e-12 of the scale absolute, cond within the bound the two eigenvalue bars imply where that is
below 0.5. On the shortcut the projection delta is exactly 0 (the reference's is the ~1e-16 rounding of
V diag(λ) Vᵀ)."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

D = 22


@pytest.fixture(scope="module")
def edges():
    import make_psd_edges as P
    return P.load()


def _check(cases, Mp, cert, what, out=None):
    import make_psd_edges as P
    bad = []
    for k, c in enumerate(cases):
        assert np.all(np.isfinite(cert[k])) and np.all(np.isfinite(Mp[k])), (what, c["name"], cert[k])
        for name, err, bound in P.bars(c, Mp[k], cert[k]):
            if out is not None:
                fam = c["name"][0]
                out.setdefault((fam, name), 0.0)
                out[(fam, name)] = max(out[(fam, name)], err / bound if bound > 0 else float(err))
            if not err <= bound:
                bad.append(f"{what} {c['name']} {name}: error {err:.3e} > bound {bound:.3e}")
    return bad


def _report(ratios, what):
    """Worst error / bar per family (printed: the figures recorded in DESIGN.md)."""
    for fam in sorted({f for f, _ in ratios}):
        print(f"{what} family {fam}: " + ", ".join(f"{n} {r:.1e}" for (f, n), r in sorted(ratios.items())
                                                   if f == fam and r > 0.0) + " (error / bar)")


@pytest.mark.parametrize("d", [22, 6, 3, 23])
def test_domain_projection_psd_at_spectrum_edges(ctx, edges, d):
    from gcslam.ops.primitives import domain_projection_psd_batch
    cs = edges[d]
    Mp, cert = domain_projection_psd_batch(np.stack([c["M"] for c in cs]), ctx=ctx)
    ratios = {}
    bad = _check(cs, Mp, cert, f"psd d={d}", ratios)
    _report(ratios, f"psd d={d}")
    assert not bad, "\n".join(bad)
    for k, c in enumerate(cs):  # the projection is symmetric to rounding
        assert np.max(np.abs(Mp[k] - Mp[k].T)) <= 1e-15 * np.max(np.abs(Mp[k])), c["name"]


def test_info_fusion_certified_projection_at_spectrum_edges(ctx, edges):
    from gcslam.ops.fusion import info_fusion_additive_batch
    cs = edges[D]
    n = len(cs)
    M = np.stack([c["M"] for c in cs])
    h = np.arange(n * D, dtype=np.float64).reshape(n, D)
    Lo, ho, cert = info_fusion_additive_batch(M, h, np.zeros_like(M), np.ones((n, D)), np.zeros(n), ctx=ctx)
    assert np.array_equal(ho, h)
    ratios = {}
    bad = _check(cs, Lo, cert, "info fusion", ratios)
    _report(ratios, "info fusion")
    assert not bad, "\n".join(bad)
    for k, c in enumerate(cs):
        if c["cert"][0] == 0.0:  # clamp inactive: the shortcut, projection = M_sym bit for bit, delta exactly 0
            assert cert[k, 0] == 0.0 and np.array_equal(Lo[k], 0.5 * (c["M"] + c["M"].T)), c["name"]


def test_barycenter_certified_projection_at_spectrum_edges(ctx, edges):
    from gcslam.ops.hypothesis import hypothesis_barycenter_batch
    cs = edges[D]
    ratios, bad = {}, []
    for c in cs:
        Lo, ho, zo, cert = hypothesis_barycenter_batch(c["M"][None], np.zeros((1, D)), np.zeros((1, D)), [1.0], 0.01,
                                                       ctx=ctx)
        bad += _check([c], Lo[None], cert[None, 5:11], "barycenter", ratios)
    _report(ratios, "barycenter")
    assert not bad, "\n".join(bad)

