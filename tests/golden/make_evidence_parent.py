"""TEST INFRASTRUCTURE — records what the photometric and the joint RGB-D pose evidence, and the accumulate and
device_out routes of the three evidences of the camera view, computed while depth_pose_evidence.py and
photometric_pose_evidence.py each held their own host driver, for the bit-identity check of
tests/test_gpu_photo_evidence.py (test_gpu_evidence_gives_the_recorded_bytes). The depth route itself is
pinned by camview_parent.npz. Run on an MI355X with the library and the Python of the commit BEFORE the two
drivers became one (91c2ae0):

    python tests/golden/make_evidence_parent.py [--force]

  evidence_parent.npz   "<route>/<case>/<array>" for every (route, case) of RUNS:
                        photo       photometric_pose_evidence_batched(return_images=True);
                        joint1, joint0   rgbd_pose_evidence_batched(return_images=True) with joint=True, False;
                        acc_depth, acc_photo, acc_joint   the three batched entries with accumulate_into, seeded
                                    non-zero (L_pose, h_pose) DeviceArrays (what comes back is their download);
                        devout_joint   rgbd_pose_evidence_batched(device_out=True), the returned DeviceArrays
                                    downloaded.
                        L_pose, h_pose and parts are kept as they are; the per-splat arrays (lum, dlum) and the
                        images (lum_render, residual, weight; the joint route's five) as the rows of "sha256":
                        the SHA-256 of the bytes of each, in the order of the route's *_DIGESTS below.

Written against the public Python API and photoev_cases only, so the same file runs before and after the
change; the test calls run below. The inputs are rebuilt from seeds by the case module, so the file holds
outputs only. The recorder refuses to overwrite an existing fixture unless given --force.
"""

from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, os.path.join(ROOT, "fl-slam_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "evidence_parent.npz")
MAX_BYTES = 100000
PHOTO_CASES = ("three_poses", "cap16", "stack", "ts8", "rgb8", "holes", "weights", "empty")
JOINT_CASES = ("three_poses", "cap16", "stack")
RUNS = tuple([("photo", n) for n in PHOTO_CASES] + [(r, n) for r in ("joint1", "joint0") for n in JOINT_CASES] +
             [(r, "three_poses") for r in ("acc_depth", "acc_photo", "acc_joint", "devout_joint")])
PHOTO_DIGESTS = ("lum", "dlum", "lum_render", "residual", "weight")
DEPTH_DIGESTS = ("residual", "weight")
JOINT_DIGESTS = ("lum", "dlum", "residual", "weight", "lum_render", "lum_residual", "lum_weight")


def _device_batch(ctx, b):
    import photoev_cases as PC
    from gcslam import rendering as R
    if b["mu_world"].shape[0] == 0:
        return R.DeviceRenderableBatch(ctx, 4, PC.CC.L)   # count = 0: no row is read
    return R.DeviceRenderableBatch.from_host(ctx, R.RenderablePrimitiveBatch(
        mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None, eta=b["eta"], mass=b["mass"],
        color=b["color"]))


def run(ctx, route, name):
    """The arrays of one (route, case): L_pose, h_pose, parts and what the route's render dict is recorded for."""
    import photoev_cases as PC
    from gcslam import _abi
    from gcslam import rendering as R
    from gcslam.ops import (DepthEvidenceConfig, PhotometricEvidenceConfig, PinholeIntrinsics, depth_pose_evidence_batched,
                            photometric_pose_evidence_batched, rgbd_pose_evidence_batched)
    c = PC.build(name)
    vcfg, pcfg, dcfg = R.CameraViewConfig(**c["cfg"]), PhotometricEvidenceConfig(**c["pcfg"]), DepthEvidenceConfig(**c["ecfg"])
    where = (_device_batch(ctx, c["batch"]), PinholeIntrinsics(*c["K"]), c["poses6"])
    camera = (c["R_bc"], c["t_bc"], vcfg)
    kind, kw = route.split("_")[-1].rstrip("01"), dict(return_images=True)
    if route.startswith("acc_"):
        P, rng = c["poses6"].shape[0], np.random.default_rng(24)
        L0, h0 = rng.normal(size=(P, 22, 22)) * 100.0, rng.normal(size=(P, 22))
        kw["accumulate_into"] = (_abi.DeviceArray.from_host(ctx, L0), _abi.DeviceArray.from_host(ctx, h0))
    if route.startswith("devout_"):
        kw["device_out"] = True
    if kind == "depth":
        got, digests = depth_pose_evidence_batched(*where, PC.depth_obs(name), *camera, dcfg, **kw), DEPTH_DIGESTS
    elif kind == "photo":
        got, digests = photometric_pose_evidence_batched(*where, c["image_obs"], *camera, pcfg, **kw), PHOTO_DIGESTS
    else:
        joint = {"joint1": True, "joint0": False}.get(route)
        got = rgbd_pose_evidence_batched(*where, PC.depth_obs(name), c["image_obs"], *camera, dcfg, pcfg, joint=joint, **kw)
        digests = JOINT_DIGESTS
    Lp, hp, parts, render = got
    if route.startswith("devout_"):
        Lp, hp = Lp.download(), hp.download()
    if route.startswith("acc_"):
        dL, dh = kw["accumulate_into"]
        assert dL.download().tobytes() == np.asarray(Lp).tobytes() and dh.download().tobytes() == np.asarray(hp).tobytes()
    out = dict(L_pose=np.asarray(Lp), h_pose=np.asarray(hp), parts=np.asarray(parts))
    return dict(out, sha256=np.stack([sha256(render[k].download()) for k in digests]))


def sha256(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def same_as_recorded(gold, key, a) -> bool:
    g, a = gold[key], np.ascontiguousarray(a)
    return g.dtype == a.dtype and g.shape == a.shape and g.tobytes() == a.tobytes()


def record(ctx):
    out = {}
    for route, name in RUNS:
        out.update({f"{route}/{name}/{k}": v for k, v in run(ctx, route, name).items()})
    return out


def main():
    if os.path.exists(OUT) and "--force" not in sys.argv[1:]:
        sys.exit(f"{OUT} exists; --force overwrites it")
    from gcslam import _abi
    out = record(_abi.default_context())
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(size, "bytes,", len(out), "arrays")
    assert size < MAX_BYTES, size
    for k, v in out.items():
        print(k, v.dtype, v.shape)


if __name__ == "__main__":
    main()
