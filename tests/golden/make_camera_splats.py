"""TEST INFRASTRUCTURE — records the reference's own outputs for the camera-splat cases into
tests/golden/camera_splats.npz.

The LiDAR depth evidence and the splat preparation are pure NumPy in the reference
(frontend/sensors/lidar_camera_depth_fusion.py, frontend/sensors/splat_prep.py, with the data types
of frontend/sensors/visual_types.py) and import without JAX. This script imports those three modules
in place (the reference tree exists only in the build container), runs

    lidar_depth_evidence(..., return_diag=True)   and   _route_b_ray_plane(...)
    splat_prep_fused(...)

on the inputs of tests/camsplat_cases.py and stores the inputs and the returned values, so the GPU
box reads the npz. Nothing here computes anything of its own.

    python tests/golden/make_camera_splats.py REFERENCE_ROOT
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import camsplat_cases as CC  # noqa: E402


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "fl_ws", "src", "fl_slam_poc"))
    from fl_slam_poc.frontend.sensors import lidar_camera_depth_fusion as F
    from fl_slam_poc.frontend.sensors.splat_prep import splat_prep_fused
    from fl_slam_poc.frontend.sensors.visual_types import ExtractionResult, Feature3D, PinholeIntrinsics
    assert "jax" not in sys.modules
    K = (CC.FX, CC.FY, CC.CX, CC.CY)
    out = {}
    for name in CC.CASES:
        c = CC.build(name)
        cfg = F.LidarCameraDepthFusionConfig(**c["cfg"])
        pre = name + "/"
        if name == "smallest":
            out[pre + "points_base"], out[pre + "points_cam"] = c["points_base"], c["points_cam"]
        else:
            out["scene/points_base"], out["scene/points_cam"] = c["points_base"], c["points_cam"]
        out[pre + "uv"] = c["uv"]
        runs = [("ref_", c["point_weights"])]
        if c["point_weights"] is not None:
            out[pre + "point_weights"] = c["point_weights"]
            runs.append(("ref_plain_", None))  # splat_prep_fused passes no weights
        for tag, pw in runs:
            L, th, diag = F.lidar_depth_evidence(c["points_cam"], c["uv"], *K, cfg, point_weights=pw, return_diag=True)
            zB, sB, wB = F._route_b_ray_plane(c["points_cam"], c["uv"], *K, cfg, point_weights=pw)
            out[pre + tag + "Lambda_ell"], out[pre + tag + "theta_ell"] = L, th
            for k, v in diag.items():
                out[pre + tag + k] = v
            out[pre + tag + "z_B"], out[pre + tag + "sigma_sq_B"], out[pre + tag + "w_B"] = zB, sB, wB
        f = c["features"]
        m = c["uv"].shape[0]
        feats = [Feature3D(u=float(f["u"][i]), v=float(f["v"][i]), xyz=f["xyz"][i].copy(), cov_xyz=f["cov_xyz"][i].copy(),
                           info_xyz=np.eye(3), logdet_cov=0.0, canonical_theta=np.zeros(3), canonical_log_partition=0.0,
                           desc=np.zeros(32, np.uint8), weight=float(f["weight"][i]),
                           meta=dict(depth_Lambda_c=float(f["depth_Lambda_c"][i]), depth_theta_c=float(f["depth_theta_c"][i])),
                           mu_app=f["mu_app"][i].copy() if f["has_mu_app"][i] else None,
                           kappa_app=float(f["kappa_app"][i]), color=f["color"][i].copy() if f["has_color"][i] else None)
                 for i in range(m)]
        fused = splat_prep_fused(ExtractionResult(features=feats, op_report=[], timestamp_ns=0), c["points_cam"],
                                 PinholeIntrinsics(*K), cfg)
        assert len(fused) == m
        out[pre + "ref_fused_xyz"] = np.array([g.xyz for g in fused], np.float64)
        out[pre + "ref_fused_cov"] = np.array([g.cov_xyz for g in fused], np.float64)
        out[pre + "ref_fused_flag"] = np.array([g is not a for g, a in zip(fused, feats)])
        for k, v in f.items():
            out[pre + "feat_" + k] = v
    dst = os.path.join(HERE, "camera_splats.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
