"""TEST INFRASTRUCTURE — records what the fused bins kernels computed before the softmax normaliser's
batched 16-lane sum (gc_binsdev.h group16_sum2) went in, for the bit-identity checks of
tests/test_gpu_bins_zbatch.py. Run on an MI355X with the library built from the commit BEFORE that change:

    python tests/golden/make_bins_zbatch_parent.py

  bins_fused_parent.npz      stats / cert of gc_scan_bins_fused (the grid form) for GRID_CASES at H = 3.
                             The geometry is fixed by iters, so the arrays do not depend on the device.
  pipeline_small_parent.npz  combined(), get_beliefs() and hyp_diag() of the batched pipeline after 2
                             scans (H = 2, 4,096 points, IMU/odom branch computed on the device): the
                             persistent k_bins_io with its window pre-pass and look-ahead tasks. Its
                             chunk geometry follows the compute-unit count, stored as "cus".

The inputs are rebuilt from seeds by the functions below (the test imports them), so the files hold
outputs only. Nothing here computes a reference: the arrays are the library's own, bit for bit.
"""

from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))
sys.path.insert(0, ROOT)

ORIGIN = np.array([-0.065447, -0.100474, 0.108987])
TWISTS = np.array([[0.02, 0.0, 0.0, 0.0, 0.0, 0.03], [0.0, 0.01, 0.0, 0.01, -0.01, -0.02], [0.0] * 6])
GRID_CASES = [(48, 777, 1), (20, 777, 1), (64, 300, 1)]  # (B, n = cap, iters)
PIPE_H, PIPE_N_AZ, PIPE_SCANS = 2, 256, 2


def scan_points(n):
    """The first n points of synthetic scan 0 (16 rings per azimuth step)."""
    from gcslam.synth import make_scan
    s = make_scan(0, n_az=(n + 15) // 16)
    assert s["points"].shape[0] >= n
    return s, s["points"][:n], s["timestamps"][:n], s["weights"][:n]


def run_fused(ctx, B, n, cap, iters, xis, tau=0.1):
    """gc_scan_bins_fused on scan_points(n): (stats (H, B, 38), cert (H, 8))."""
    from gcslam import _abi
    from oracle import gc_oracle as O
    s, P, T, W = scan_points(n)
    H = xis.shape[0]
    dP, dT, dW = (_abi.DeviceArray.from_host(ctx, a) for a in (P, T, W))
    scal = _abi.DeviceArray(ctx, 8)
    _abi.call("gc_budget_stats", ctx.handle, dW.ptr, n, cap, scal.ptr, ctx=ctx)
    dX, dB = _abi.DeviceArray.from_host(ctx, xis), _abi.DeviceArray.from_host(ctx, O.fibonacci_atlas(B))
    st, ce = _abi.DeviceArray(ctx, (H, B, 38)), _abi.DeviceArray(ctx, (H, 8))
    oa, op = _abi.f64p(ORIGIN)
    _abi.call("gc_scan_bins_fused", ctx.handle, H, n, cap, B, dP.ptr, dT.ptr, dW.ptr, scal.ptr, s["scan_start"],
              s["scan_end"], dX.ptr, dB.ptr, tau, op, 1e-12, 1e-12, st.ptr, ce.ptr, iters, ctx=ctx)
    return st.download(), ce.download()


def run_pipeline(ctx):
    """The small pipeline case: {name: array} of combined(), get_beliefs() and hyp_diag() after the scans."""
    from gcslam.pipeline import BatchedScanPipeline, PipelineConfig
    from oracle import cases
    case = cases.build(H=PIPE_H, n_az=PIPE_N_AZ, n_scans=PIPE_SCANS, io="computed")
    pipe = BatchedScanPipeline(PIPE_H, case["n"], PipelineConfig(n_points_cap=case["n"]), ctx=ctx)
    hy = case["hyp"]
    pipe.set_beliefs(hy["X_anchor"], hy["z_lin"], hy["L"], hy["h"], hy["stamp"])
    pipe.set_weights(hy["weights"])
    pipe.set_io_mode(True)
    pipe.set_iw(*case["iw"])
    pipe.set_map(case["map_record"])
    for k, s in enumerate(case["scans"]):
        pipe.stage_scan(0, s)
        pipe.run_scan(0, s, case["state"].scan_count + k)
    ctx.sync()
    out = {"combined_" + k: np.asarray(v) for k, v in pipe.combined().items()}
    out.update({"belief_" + k: np.asarray(v) for k, v in pipe.get_beliefs().items()})
    out["hyp_diag"] = np.asarray(pipe.hyp_diag())
    return out


def device_cus(device=0):
    """Compute units of the device (hipDeviceAttributeMultiprocessorCount)."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")  # the library's own rpath (fl-slam_amd/Makefile)
    v = ctypes.c_int(0)
    rc = hip.hipDeviceGetAttribute(ctypes.byref(v), 63, int(device))
    if rc != 0:
        raise RuntimeError(f"hipDeviceGetAttribute failed: {rc}")
    return int(v.value)


def main():
    from gcslam import _abi
    ctx = _abi.default_context()
    grid = {}
    for B, n, iters in GRID_CASES:
        st, ce = run_fused(ctx, B, n, n, iters, TWISTS)
        grid[f"stats_B{B}_n{n}_i{iters}"], grid[f"cert_B{B}_n{n}_i{iters}"] = st, ce
    np.savez_compressed(os.path.join(HERE, "bins_fused_parent.npz"), **grid)
    pipe = run_pipeline(ctx)
    pipe["cus"] = np.array(device_cus(ctx.device))
    np.savez_compressed(os.path.join(HERE, "pipeline_small_parent.npz"), **pipe)
    for name, d in (("bins_fused_parent", grid), ("pipeline_small_parent", pipe)):
        assert all(np.all(np.isfinite(v)) for v in d.values()), name  # np.array_equal must be able to hold
        print(name, {k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
