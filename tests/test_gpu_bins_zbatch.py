"""The fused bins kernels with the softmax normaliser's batched 16-lane sum (gc_binsdev.h group16_sum2;
B = 16 keeps the per-step butterfly, group16_sum): every instantiation of the grid form against the oracle
chain, and bit identity with what the library computed before the batched form existed
(tests/golden/bins_fused_parent.npz, pipeline_small_parent.npz; recorded by
tests/golden/make_bins_zbatch_parent.py). The batched sum adds the same partials in the same
association, so the outputs are the recorded bits. The build switch that selected between these forms, the
batch of four and the swizzle sums was removed; the last commit whose tree holds them is dd48cdd, their
measurements are in profiles/r07/ab_bins_zbatch.txt and profiles/r06/ab_zsum_swizzle.txt.

The late-ticket instantiation of k_bins_io (H = 256) is too large for a test of seconds: its outputs are
compared byte for byte with bench.py --dump-outputs (profiles/r07/ab_bins_zbatch.txt)."""

import os

import numpy as np
import pytest

from oracle import gc_oracle as O
from tests.golden import make_bins_zbatch_parent as G

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAST = np.array([[0.3, -0.1, 0.05, 0.3, -0.2, 0.4],      # |ω| 0.54: short, then the series
                 [0.1, 0.0, 0.2, 1.2, 0.5, -0.9],        # |ω| 1.58: all three forms
                 [-0.5, 0.4, 0.0, -2.5, 1.0, 2.0]])      # |ω| 3.35: mostly the closed form
TAU = 0.1


def _check_stats(stats, cert, ref, rtol=1e-10):
    """tests/test_gpu_points.py _check_stats, bar for bar."""
    from gcslam.ops.binning import unpack_bin_stats
    u = unpack_bin_stats(stats)
    scale = max(np.max(np.abs(ref["N"])), 1e-300)
    np.testing.assert_allclose(u["N"], ref["N"], atol=rtol * scale, rtol=0)
    np.testing.assert_allclose(u["s_dir"], ref["s_dir"], atol=rtol * scale, rtol=0)
    np.testing.assert_allclose(u["S_dir_scatter"], ref["S_dir_scatter"], atol=rtol * scale, rtol=0)
    np.testing.assert_allclose(u["p_bar"], ref["p_bar"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(u["Sigma_p"], ref["Sigma_p"], atol=1e-8, rtol=0)
    np.testing.assert_allclose(u["kappa"], ref["kappa"], rtol=1e-8, atol=1e-10)
    assert abs(cert[0] - ref["ess"]) <= 1e-9 * ref["ess"]
    assert abs(cert[1] - ref["support_frac"]) < 1e-12
    assert abs(cert[2] - ref["psd_delta"]) < 1e-8
    assert abs(cert[3] - ref["max_eps_ratio"]) <= 1e-9 * ref["max_eps_ratio"] + 1e-300


_DESKEWED = {}


def _deskewed(n, cap, key, xis):
    """Oracle budget -> deskew -> directions of scan_points(n), once per (n, cap, twist set): the bins
    do not enter before the soft assignment."""
    k = (n, cap, key)
    if k not in _DESKEWED:
        s, P, T, W = G.scan_points(n)
        bud = O.point_budget_resample(P, T, W, None, None, cap)
        per = []
        for xi in xis:
            p0, wd, ret = O.deskew_constant_twist(bud["points"], bud["timestamps"], bud["weights"], s["scan_start"],
                                                  s["scan_end"], xi)
            per.append((p0, wd, ret, O.point_directions(p0, G.ORIGIN)))
        _DESKEWED[k] = (bud["weights"].sum(), per)
    return _DESKEWED[k]


def _fused_vs_chain(ctx, B, n, cap, iters, key, xis):
    stats, cert = G.run_fused(ctx, B, n, cap, iters, xis, TAU)
    wsum, per = _deskewed(n, cap, key, xis)
    bins = O.fibonacci_atlas(B)
    for h, (p0, wd, ret, dirs) in enumerate(per):
        sa = O.bin_soft_assign(dirs, bins, TAU)
        ref = O.scan_bin_moment_match(p0, None, wd, sa["resp"], None, G.ORIGIN)
        _check_stats(stats[h], cert[h], ref, rtol=1e-10)
        # the logits round at ulp(1/τ): entropy within ~B·ulp(1/τ), max responsibility within a few ulp(1/τ)
        assert abs(cert[h, 4] - sa["avg_entropy"]) < 1e-9 + 48 * np.spacing(1.0 / TAU)
        assert abs(cert[h, 5] - sa["max_resp"]) < 1e-12 + 4 * np.spacing(1.0 / TAU)
        assert abs(cert[h, 6] / (wsum + 1e-12) - ret) < 1e-12


@pytest.mark.parametrize("B", [9, 16, 20, 32, 40, 48, 55, 64])
def test_every_instantiation_matches_contract_chain(ctx, B):
    """1 to 4 bins per lane, each with every bin lane full (B = 16, 32, 48, 64) and with masked lanes; 777
    points at one iteration per task: three full 256-point chunks and a 9-point padded one, so both the
    unpadded and the padded specialisation of the step loop run."""
    _fused_vs_chain(ctx, B, 777, 777, 1, "twists", G.TWISTS)


def test_fast_rotation_matches_contract_chain(ctx):
    _fused_vs_chain(ctx, 48, 777, 777, 1, "fast", FAST)


def test_task_of_two_iterations_matches_contract_chain(ctx):
    """1000 points at two iterations per task: a full task and a padded one (488 points), each running the
    step loop twice (Π Z and the accumulators carried across iterations)."""
    _fused_vs_chain(ctx, 48, 1000, 1000, 2, "twists", G.TWISTS)


@pytest.mark.parametrize("B,n,iters", G.GRID_CASES)
def test_grid_form_is_bit_identical_with_parent(ctx, B, n, iters):
    g = np.load(os.path.join(GOLD, "bins_fused_parent.npz"))
    stats, cert = G.run_fused(ctx, B, n, n, iters, G.TWISTS, TAU)
    assert np.array_equal(stats, g[f"stats_B{B}_n{n}_i{iters}"])
    assert np.array_equal(cert, g[f"cert_B{B}_n{n}_i{iters}"])


def test_pipeline_form_is_bit_identical_with_parent(ctx):
    """k_bins_io (persistent tasks, the window pre-pass, the look-ahead instantiation) through two scans of
    the small pipeline. The chunk geometry, hence the summation order, follows the compute-unit count."""
    g = np.load(os.path.join(GOLD, "pipeline_small_parent.npz"))
    cus = G.device_cus(ctx.device)
    if cus != int(g["cus"]):
        pytest.skip(f"recorded on a device with {int(g['cus'])} compute units, this one has {cus}: "
                    "another chunk geometry, another summation order")
    out = G.run_pipeline(ctx)
    assert sorted(out) == sorted(k for k in g.files if k != "cus")
    for k, v in out.items():
        assert np.array_equal(v, g[k]), k
