"""TEST INFRASTRUCTURE — records what the camera view and the depth pose evidence computed while each of
csrc/gc_camrender.hip and csrc/gc_depthev.hip held its own copy of the projection, the view packing and
the raster step, for the bit-identity check of tests/test_gpu_camera_render.py
(test_gpu_camera_view_gives_the_recorded_bytes). Run on an MI355X with the library built from the commit
BEFORE those copies became one (da741bf):

    python tests/golden/make_camview_parent.py [--force]

  camview_parent.npz   "cam/<case>/<array>" for the camrender_cases CAM_CASES: every array of gc_cam_splats
                       (means_px, Sigmas_inv, depths, radii, alphas, colors, valid) and of
                       gc_render_depth_tiles (images, alpha, depth, n_contrib, tile_counts, tile_survivors,
                       tile_indices);
                       "ev/<case>/<array>" for the depthev_cases EV_CASES through
                       depth_pose_evidence_batched(return_images=True): dmeans_px, ddepths, dSigmas_inv,
                       L_pose, h_pose, parts, residual, weight.

Written against the public Python API and the test cases only, so the same file runs before and after the
change; the test calls run_cam and run_ev below. The inputs are rebuilt from seeds by the case modules, so
the file holds outputs only. Arrays are compared as bytes: the +inf depth of an invalid splat is part of
the record.

The file has to stay below the largest fixture here (ops.npz, MAX_BYTES), and random mantissas do not
deflate, so the arrays are packed without loss (pack; recorded puts them back):
  "<array>__planes"   a float64 array as its eight byte planes (shape (8,) + the array's: plane b holds byte b
                      of every value) where that deflates to less, as the sign and exponent planes usually do;
  "<array>__rows_of"  the name of an earlier array whose leading rows are this array's bytes (the tangents of
                      `holes` are those of pose 0 of `three_poses`: the same scene and pose);
  "<array>__sha256"   the SHA-256 of the bytes of a colour `images` array, and of nothing else, where the file
                      would not fit with the images themselves (it did not: 934,096 bytes with them).
The recorder refuses to overwrite an existing fixture unless given --force. --pack RAW.npz packs the arrays
of an earlier recording (np.savez of what record returns) instead of asking the device again; the committed
file is the packing of the one recording made on an MI355X at da741bf.
"""

from __future__ import annotations

import hashlib
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, os.path.join(ROOT, "fl-slam_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "camview_parent.npz")
MAX_BYTES = 646225  # ops.npz
CAM_CASES = ("two_views", "stack", "invalid", "cap16", "three_views_ts8")
EV_CASES = ("three_poses", "ts8", "stack", "holes", "cap16")
EV_ARRAYS = ("dmeans_px", "ddepths", "dSigmas_inv", "residual", "weight")
DIGEST, PLANES, ROWS_OF = "__sha256", "__planes", "__rows_of"


def _device_batch(ctx, b):
    from gcslam import rendering as R
    return R.DeviceRenderableBatch.from_host(ctx, R.RenderablePrimitiveBatch(
        mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None, eta=b["eta"], mass=b["mass"],
        color=b["color"]))


def run_cam(ctx, name, views=None):
    """The splats and the composite of a camrender case; views: indices into the case's views, repeats allowed."""
    import camrender_cases as CC
    from gcslam import rendering as R
    from gcslam.ops import PinholeIntrinsics
    c = CC.build(name)
    sel = range(len(c["Ks"])) if views is None else views
    Ks, T = [PinholeIntrinsics(*c["Ks"][v]) for v in sel], np.stack([c["T_cws"][v] for v in sel])
    cfg = R.CameraViewConfig(**c["cfg"])
    splats = R.camera_splat_prep(_device_batch(ctx, c["batch"]), Ks, T, c["H"], c["W"], cfg)
    dev = R.render_depth_tiles(splats, c["H"], c["W"], cfg, ctx=ctx)
    return {k: v.download() for k, v in dict(splats, **dev).items()}


def run_ev(ctx, name):
    import depthev_cases as DC
    from gcslam import rendering as R
    from gcslam.ops import DepthEvidenceConfig, PinholeIntrinsics, depth_pose_evidence_batched
    c = DC.build(name)
    Lp, hp, parts, render = depth_pose_evidence_batched(
        _device_batch(ctx, c["batch"]), PinholeIntrinsics(*c["K"]), c["poses6"], c["depth_obs"], c["R_bc"], c["t_bc"],
        R.CameraViewConfig(**c["cfg"]), DepthEvidenceConfig(**c["ecfg"]), return_images=True)
    out = {k: render[k].download() for k in EV_ARRAYS}
    return dict(out, L_pose=np.asarray(Lp), h_pose=np.asarray(hp), parts=np.asarray(parts))


def sha256(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def planes(a) -> np.ndarray:
    return np.ascontiguousarray(np.moveaxis(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), -1, 0))


def _deflated(a) -> int:
    return len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6))


def pack(out, digest_images: bool):
    """The entries of the file for the recorded arrays `out`, in their order."""
    packed, seen = {}, []
    for k, a in out.items():
        a = np.ascontiguousarray(a)
        same = [o for o in seen if out[o].dtype == a.dtype and out[o].shape[1:] == a.shape[1:] and a.nbytes >= 1024 and
                out[o][:a.shape[0]].tobytes() == a.tobytes()]
        if digest_images and k.startswith("cam/") and k.endswith("/images"):
            packed[k + DIGEST] = sha256(a)
        elif same:
            packed[k + ROWS_OF] = np.array(same[0])
        elif a.dtype == np.float64 and _deflated(planes(a)) < _deflated(a):
            packed[k + PLANES] = planes(a)
        else:
            packed[k] = a
        seen.append(k)
    return packed


def recorded(gold, key) -> np.ndarray:
    """The array recorded under key (not one stored as a digest)."""
    if key + ROWS_OF in gold.files:
        return recorded(gold, str(gold[key + ROWS_OF]))
    if key + PLANES in gold.files:
        g = gold[key + PLANES]
        return np.ascontiguousarray(np.moveaxis(g, 0, -1)).view(np.float64).reshape(g.shape[1:])
    return gold[key]


def recorded_keys(gold) -> set:
    """The names of the recorded arrays, however each is stored."""
    return {next((k[:-len(s)] for s in (DIGEST, PLANES, ROWS_OF) if k.endswith(s)), k) for k in gold.files}


def same_as_recorded(gold, key, a) -> bool:
    """a against what was recorded under key, or against its digest where the recorder stored one."""
    a = np.ascontiguousarray(a)
    if key + DIGEST in gold.files:
        return gold[key + DIGEST].tobytes() == sha256(a).tobytes()
    g = recorded(gold, key)
    if key + ROWS_OF in gold.files:
        g = g[:a.shape[0]]
    return g.dtype == a.dtype and g.shape == a.shape and g.tobytes() == a.tobytes()


def record(ctx):
    out = {}
    for name in CAM_CASES:
        out.update({f"cam/{name}/{k}": v for k, v in run_cam(ctx, name).items()})
    for name in EV_CASES:
        out.update({f"ev/{name}/{k}": v for k, v in run_ev(ctx, name).items()})
    return out


def main():
    args = sys.argv[1:]
    if os.path.exists(OUT) and "--force" not in args:
        sys.exit(f"{OUT} exists; --force overwrites it")
    if "--pack" in args:
        raw = np.load(args[args.index("--pack") + 1])
        out = {k: raw[k] for k in raw.files}
    else:
        from gcslam import _abi
        out = record(_abi.default_context())
    for digest_images in (False, True):
        np.savez_compressed(OUT, **pack(out, digest_images))
        size = os.path.getsize(OUT)
        print(size, "bytes with the colour images as", "digests" if digest_images else "arrays")
        if size < MAX_BYTES:
            break
    assert size < MAX_BYTES, size
    print(len(out), "arrays")
    for k, v in out.items():
        print(k, v.dtype, v.shape)


if __name__ == "__main__":
    main()
