"""The camera view on the device (gc_camrender.hip, gcslam/rendering.py) against the restatement
(tests/camrender_restatement.py) on the seeded cases (tests/camrender_cases.py), whose conditions
tests/test_camera_render.py asserts.

Lists, counts, survivors, n_contrib and valid are compared exactly. Float fields: max |difference| over
the field <= 1e-10 of the field's max-abs over the case (the camera-feature tests' bar: condition numbers
of Sigma_px <= 100, exponents q / 2 <= a few tens, at most 256 terms per pixel). The measured worst
fractions are printed and recorded in DESIGN.md §4."""

import ctypes

import numpy as np
import pytest

import camrender_cases as CC
import render_cases as RC
from gcslam import _abi
from gcslam import rendering as R
from gcslam.ops.camera_splats import PinholeIntrinsics

PREP_FLOATS = ("means_px", "Sigmas_inv", "depths", "radii", "alphas", "colors")
IMAGE_FLOATS = ("images", "alpha", "depth")
EXACT = ("valid", "n_contrib", "tile_counts", "tile_survivors", "tile_indices")
BAR = 1e-10


def _host_batch(b):
    return R.RenderablePrimitiveBatch(mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None,
                                      eta=b["eta"], mass=b["mass"], color=b["color"])


def _device_batch(ctx, b):
    if b["mu_world"].shape[0] == 0:
        return R.DeviceRenderableBatch(ctx, 4, CC.L)   # count = 0: no row is read
    return R.DeviceRenderableBatch.from_host(ctx, _host_batch(b))


def _args(c):
    return [PinholeIntrinsics(*k) for k in c["Ks"]], np.stack(c["T_cws"]), c["H"], c["W"], R.CameraViewConfig(**c["cfg"])


def _run(ctx, name):
    c = CC.build(name)
    Ks, T, h, w, cfg = _args(c)
    splats = R.camera_splat_prep(_device_batch(ctx, c["batch"]), Ks, T, h, w, cfg)
    dev = R.render_depth_tiles(splats, h, w, cfg, ctx=ctx)
    return {k: v.download() for k, v in dict(splats, **dev).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CC.CASES))
def test_gpu_camera_parity(ctx, name):
    want, _ = CC.restated(name)
    got = _run(ctx, name)
    for k in EXACT:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    worst = {k: CC.err_frac(got[k], want[k]) for k in PREP_FLOATS + IMAGE_FLOATS}
    print(name, "worst difference / max-abs:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= BAR, worst
    # the composed call gives the same bytes from a host batch
    c = CC.build(name)
    if c["batch"]["mu_world"].shape[0]:
        Ks, T, h, w, cfg = _args(c)
        out = R.render_map_camera(_host_batch(c["batch"]), Ks, T, h, w, cfg, ctx=ctx)
        for k in IMAGE_FLOATS + EXACT[1:]:
            assert getattr(out, k).tobytes() == got[k].tobytes(), k
        assert set(out.device) >= set(PREP_FLOATS + IMAGE_FLOATS + EXACT)


@pytest.mark.gpu
def test_gpu_camera_reproducible_and_no_carry_over(ctx):
    """Two calls give identical bytes; a call with few primitives after one with many gives the bytes it
    gave before it (nothing left in scratch, lists or images)."""
    small = _run(ctx, "stack")
    big = _run(ctx, "cap256")
    again = _run(ctx, "cap256")
    for k in big:
        assert big[k].tobytes() == again[k].tobytes(), k
    after = _run(ctx, "stack")
    for k in small:
        assert small[k].tobytes() == after[k].tobytes(), k
    empty = _run(ctx, "empty")
    assert (empty["tile_indices"] == -1).all() and not empty["tile_survivors"].any() and not empty["alpha"].any()


def _device_map(ctx, tiles):
    from gcslam.primitive_map import DevicePrimitiveMap
    from oracle import gc_oracle as O
    keys = list(tiles)
    dm = DevicePrimitiveMap(len(keys), RC.M_TILE, ctx=ctx)
    dm.set_tile_keys(keys)
    full = {k: np.concatenate([tiles[kk][k] for kk in keys]) for k in O.empty_tile(1, RC.L)}
    full["valid_mask"] = full["valid_mask"].astype(np.uint8)
    dm.upload(**full)
    return dm


@pytest.mark.gpu
def test_gpu_render_map_camera_from_a_device_map(ctx):
    """Three small tiles (empty, full, half full), seen from 8 m back along z through a slightly turned
    camera given as the project's 6-vector: the bytes of the path through publish_renderable and a host
    round trip of the batch."""
    from oracle import gc_oracle as O
    dm = _device_map(ctx, RC.build_map())
    pose = np.array([0.3, -0.2, -8.0, 0.02, -0.03, 0.05])
    T_cw = R.camera_from_world(pose, ctx=ctx)
    Rwb = O.so3_exp(pose[3:])
    np.testing.assert_allclose(T_cw[:3, :3], Rwb.T, atol=1e-12)
    np.testing.assert_allclose(T_cw[:3, 3], -Rwb.T @ pose[:3], atol=1e-12)
    K = PinholeIntrinsics(40.0, 40.0, 16.0, 16.0)
    cfg = R.CameraViewConfig(max_splats_per_tile=32)
    a = R.render_map_camera(dm, K, T_cw, 32, 32, cfg)
    host = R.publish_renderable(dm).download()
    assert host.mu_world.shape[0] == RC.M_TILE + RC.M_TILE // 2
    b = R.render_map_camera(host, K, T_cw, 32, 32, cfg, ctx=ctx)
    for k in IMAGE_FLOATS + EXACT[1:]:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert a.alpha.max() > 0.3 and a.n_contrib.max() >= 3 and np.isfinite(a.images).all()
    assert 4.0 < a.depth[a.alpha > 0.3].min() and a.depth.max() < 12.0
    assert a.tile_survivors.max() > 0 and (a.tile_counts <= 32).all()


@pytest.mark.gpu
def test_gpu_render_map_bev_gives_the_recorded_bytes(ctx):
    """render_map_bev on its image case: the bytes the build gave before the tile selection and the
    shading moved into the header the camera view shares (tests/golden/render_bev_parent.npz)."""
    import os
    gold = np.load(os.path.join(os.path.dirname(RC.GOLDEN), "render_bev_parent.npz"))
    I = RC.IMAGE
    vp = R.Viewport(I["origin_xy"], I["px_per_m"], I["H"], I["W"])
    cfg = R.SplatRenderingConfig(**RC.RENDER_CFG)
    bcfg = R.BEVPushforwardConfig(oblique_phi_deg=I["oblique_phi_deg"], n_views=I["n_views"],
                                  phi_center_deg=I["phi_center_deg"], phi_span_deg=I["phi_span_deg"])
    b = RC.build_image_batch()
    batch = R.RenderablePrimitiveBatch(mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None,
                                       eta=b["eta"], mass=b["mass"], color=b["color"], primitive_ids=b["primitive_ids"])
    for views in ("bev15", "single"):
        a = R.render_map_bev(batch, vp, cfg, bcfg, views, fbm_seed=I["fbm_seed"],
                             fbm_modulate_scale=I["fbm_modulate_scale"], ctx=ctx)
        for k in ("means_px", "Sigmas_inv", "alphas", "colors"):
            assert a.device[k].download().tobytes() == gold[k + "_" + views].tobytes(), (views, k)
        assert a.tile_counts.tobytes() == gold["tile_counts_" + views].tobytes()
        assert a.tile_indices.tobytes() == gold["tile_indices_" + views].tobytes()
        assert a.images.tobytes() == gold["images_" + views].tobytes(), views


@pytest.mark.gpu
def test_gpu_camera_view_gives_the_recorded_bytes(ctx):
    """The camera view and the depth evidence on their recorded cases: the bytes the build gave while
    gc_camrender.hip and gc_depthev.hip each held their own projection, view packing and raster step
    (tests/golden/camview_parent.npz, recorded by make_camview_parent.py before they moved into
    gc_renderdev.h). And the split of the views over launches leaves no trace: one view more than a launch
    carries (kCamViewsPerLaunch = 16), all of them the first view of two_views, give that view's bytes."""
    from tests.golden import make_camview_parent as MP
    gold = np.load(MP.OUT)
    seen = set()
    for group, names, run in (("cam", MP.CAM_CASES, MP.run_cam), ("ev", MP.EV_CASES, MP.run_ev)):
        for name in names:
            for k, a in run(ctx, name).items():
                key = f"{group}/{name}/{k}"
                assert MP.same_as_recorded(gold, key, a), key
                seen.add(key)
    assert seen == MP.recorded_keys(gold) and len(seen) == 5 * 14 + 5 * 8
    one, other = MP.run_cam(ctx, "two_views", views=[0]), MP.run_cam(ctx, "two_views", views=[1])
    assert MP.same_as_recorded(gold, "cam/two_views/depth", np.concatenate([one["depth"], other["depth"]]))
    many = MP.run_cam(ctx, "two_views", views=[0] * 17)
    for k, a in many.items():
        if k == "alphas":  # per primitive, the same for every view
            assert a.tobytes() == one[k].tobytes()
            continue
        assert a.shape[0] == 17, k
        for v in range(17):
            assert a[v].tobytes() == one[k][0].tobytes(), (k, v)


@pytest.mark.gpu
def test_gpu_camera_entry_argument_errors(ctx):
    """The C entries reject what the Python layer rejects, before any launch; the context stays usable."""
    z = _abi.DeviceArray(ctx, (64,), np.float64)
    zi = _abi.DeviceArray(ctx, (64,), np.int32)
    zb = _abi.DeviceArray(ctx, (64,), np.uint8)
    batch = R._BatchStruct(3, 0, *([z.ptr] * 8))
    st = R._CamSplatStruct(z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, zb.ptr)

    def with_cfg(name, v):
        h = R._camview_cfg(R.CameraViewConfig())
        getattr(h, name)  # a member of gc_camview_cfg
        setattr(h, name, v)
        return h
    cfg0 = R._camview_cfg(R.CameraViewConfig())

    def prep(n=1, nv=1, T=None, K=(60.0, 60.0, 32.0, 24.0), H=48, W=64, cfg=None, lobes=3):
        T = np.ascontiguousarray(np.tile(np.eye(4), (max(nv, 1), 1, 1)) if T is None else T, np.float64)
        K = np.ascontiguousarray(np.tile(np.asarray(K, np.float64), (max(nv, 1), 1)))
        h = cfg0 if cfg is None else cfg
        bs = R._BatchStruct(lobes, 0, *([z.ptr] * 8))
        _abi.call("gc_camera_splat_prep", ctx.handle, ctypes.byref(bs), n, nv, T.ctypes.data, K.ctypes.data, H, W,
                  ctypes.byref(h), ctypes.byref(st), ctx=ctx)
    bottom, skew, nanT = np.eye(4), np.eye(4), np.eye(4)
    bottom[3, 2], skew[0, 1], nanT[0, 3] = 0.5, 1e-6, np.nan
    for kw in (dict(n=-1), dict(n=(1 << 24) + 1), dict(nv=0), dict(nv=33), dict(lobes=0), dict(lobes=9), dict(H=0),
               dict(W=16385), dict(K=(0.0, 60.0, 32.0, 24.0)), dict(K=(60.0, -2.0, 32.0, 24.0)),
               dict(K=(60.0, 60.0, np.nan, 24.0)), dict(T=bottom[None]), dict(T=skew[None]), dict(T=nanT[None]),
               dict(cfg=with_cfg("near", 0.0)), dict(cfg=with_cfg("far", 0.1)), dict(cfg=with_cfg("alpha_max", 0.0)),
               dict(cfg=with_cfg("alpha_max", 1.5)), dict(cfg=with_cfg("lowpass_px2", np.nan)),
               dict(cfg=with_cfg("t_stop", np.inf))):
        with pytest.raises(ValueError):
            prep(**kw)

    def tiles(n=1, nv=1, H=32, W=32, ts=16, cap=4, cfg=None):
        h = cfg0 if cfg is None else cfg
        _abi.call("gc_render_depth_tiles", ctx.handle, nv, n, ctypes.byref(st), H, W, ts, cap, ctypes.byref(h), z.ptr, z.ptr,
                  z.ptr, zi.ptr, zi.ptr, zi.ptr, zi.ptr, ctx=ctx)
    for kw in (dict(ts=0), dict(ts=33), dict(H=40), dict(W=24), dict(H=0), dict(cap=0), dict(cap=257), dict(n=-1),
               dict(nv=0), dict(nv=33), dict(cfg=with_cfg("near", -1.0)), dict(cfg=with_cfg("alpha_max", 2.0)),
               dict(cfg=with_cfg("alpha_skip", np.nan)), dict(n=1 << 24, nv=32, H=16384, W=16384)):
        with pytest.raises(ValueError):
            tiles(**kw)
    # the context is usable afterwards: n = 0 through the entry gives empty lists and the background
    img = _abi.DeviceArray(ctx, (2, 8, 16, 3), np.float64)
    al, dp = _abi.DeviceArray(ctx, (2, 8, 16), np.float64), _abi.DeviceArray(ctx, (2, 8, 16), np.float64)
    nc = _abi.DeviceArray(ctx, (2, 8, 16), np.int32)
    cnt, sv, idx = (_abi.DeviceArray(ctx, s, np.int32) for s in ((2, 2), (2, 2), (2, 2, 4)))
    for a in (img, al, dp):
        a.upload(np.ones(a.shape))
    for a in (nc, cnt, sv, idx):
        a.upload(np.ones(a.shape, np.int32))
    h = with_cfg("bg_r", 0.5)
    _abi.call("gc_render_depth_tiles", ctx.handle, 2, 0, None, 8, 16, 8, 4, ctypes.byref(h), img.ptr, al.ptr, dp.ptr, nc.ptr,
              cnt.ptr, sv.ptr, idx.ptr, ctx=ctx)
    want = np.zeros(img.shape)
    want[..., 0] = 0.5
    assert np.array_equal(img.download(), want) and not al.download().any() and not dp.download().any()
    assert not nc.download().any() and not cnt.download().any() and not sv.download().any()
    assert (idx.download() == -1).all()
