"""Rendering on the device (gc_render.hip, gcslam/rendering.py) against the outputs the reference's own
NumPy code gave for the same inputs (tests/golden/render.npz) and, for what the reference leaves
unpinned (the composition of render_map_bev and the publisher's batch from an atlas view), against
the restatement (tests/render_restatement.py) and the oracle's extract_atlas_map_view. The conditions
under which the cases pin an implementation are asserted in test_render.py.

Index lists, counts, batch order and primitive ids are compared exactly. Tile drop-in images and fBm
values: max |difference| <= 1e-12 (colours lie in [0, 1] and a pixel is a convex combination, so the
error is about twice the worst relative error of a weight: that of exp's argument, <= 25 x a few ulp,
plus exp's own ulp, plus <= 256 summation roundings). Prep outputs: 1e-12 of each field's max
(condition numbers <= 100). Composed images: 1e-10 (the Sigma^-1 error is multiplied by
q <= 2 log_clip in the exponent). The measured values are printed and recorded in DESIGN.md §4."""

import ctypes

import numpy as np
import pytest

import render_cases as RC
import render_restatement as RS
from gcslam import _abi
from gcslam import rendering as R

TILES = list(RC.TILE_CASES)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(RC.GOLDEN))


@pytest.fixture(scope="module")
def restated():
    return {False: RC.restated_image(False), True: RC.restated_image(True)}


def _tile(gold, name):
    pre = "tile/" + name + "/"
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", TILES)
def test_gpu_tile_dropins(ctx, gold, name):
    c, g = RC.build_tile(name), _tile(gold, name)
    idx = R.splat_indices_for_tile(c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["cap"], ctx=ctx)
    assert idx.dtype == np.int64
    np.testing.assert_array_equal(idx, g["ref_indices"])
    args = (c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["alphas"], c["colors"])
    worst = RC.err(R.render_tile_ewa(*args, splat_indices=g["ref_indices"], ctx=ctx), g["ref_image"])
    if "ref_image_none" in g:
        worst = max(worst, RC.err(R.render_tile_ewa(*args, ctx=ctx), g["ref_image_none"]))
    if "ref_image_empty" in g:
        assert not R.render_tile_ewa(*args, splat_indices=np.array([], np.int64), ctx=ctx).any()
    if "ref_image_fbm" in g:
        f = RC.FBM_TILE
        got = R.render_tile_ewa(*args, splat_indices=g["ref_indices"], means_world_xy=c["world_xy"],
                                fbm_octaves=f["octaves"], fbm_gain=f["gain"], fbm_seed=f["seed"],
                                fbm_modulate_scale=f["scale"], ctx=ctx)
        assert RC.err(got, g["ref_image"]) > 1e-3  # the modulation is visible
        worst = max(worst, RC.err(got, g["ref_image_fbm"]))
    print(name, "tile image, worst |difference|: %.3g" % worst)
    assert worst <= 1e-12


@pytest.mark.gpu
def test_gpu_tile_bins_above_the_lds_cap(ctx):
    """max_splats_per_tile above 256 (the one-tile drop-in alone allows it) takes the sort path, 256 and
    below the per-tile selection: the same lists."""
    c = RC.build_tile("t32_n257")
    for cap in (300, 256, 100):
        want, cd = RS.tile_bins(c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], cap)
        assert cd["margin"] >= 1e-9 and cd["gap"] >= 1e-9 and cd["ties"] == 0 and cd["survivors"] > 100
        got = R.splat_indices_for_tile(c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], cap, ctx=ctx)
        np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_gpu_fbm(ctx, gold):
    worst = 0.0
    for octaves, seed in RC.FBM_RUNS:
        got = R.fbm_at_splat_positions(gold["fbm/xy"], octaves=octaves, gain=RC.FBM_GAIN, seed=seed, ctx=ctx)
        worst = max(worst, RC.err(got, gold[f"fbm/ref_o{octaves}_s{seed}"]))
    print("fbm, worst |difference|: %.3g" % worst)
    assert worst <= 1e-12


def _host_batch(b):
    return R.RenderablePrimitiveBatch(mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None,
                                      eta=b["eta"], mass=b["mass"], color=b["color"], primitive_ids=b["primitive_ids"])


def _image_cfgs():
    I = RC.IMAGE
    return (R.Viewport(I["origin_xy"], I["px_per_m"], I["H"], I["W"]), R.SplatRenderingConfig(**RC.RENDER_CFG),
            R.BEVPushforwardConfig(oblique_phi_deg=I["oblique_phi_deg"], n_views=I["n_views"],
                                   phi_center_deg=I["phi_center_deg"], phi_span_deg=I["phi_span_deg"]))


@pytest.mark.gpu
def test_gpu_bev_splat_prep(ctx, gold, restated):
    b = RC.build_image_batch()
    vp, cfg, bcfg = _image_cfgs()
    P, vd = R.bev_views(bcfg, "bev15")
    dev = R.bev_splat_prep(R.DeviceRenderableBatch.from_host(ctx, _host_batch(b)), vp, P, vd, cfg,
                           fbm_seed=RC.IMAGE["fbm_seed"], fbm_modulate_scale=RC.IMAGE["fbm_modulate_scale"],
                           with_sigma_bev=True)
    got = {k: v.download() for k, v in dev.items()}
    worst = {}
    for k in ("means_px", "Sigmas_inv", "alphas", "colors", "Sigmas_bev"):
        want = np.stack([s[k] for s in restated[False]["splats"]])
        worst[k] = RC.err_rel(got[k], want)
    worst["fbm"] = RC.err(got["fbm"], restated[False]["splats"][0]["fbm"])
    m = RC.PREP_ROWS  # and the reference's own pushforward where it was recorded
    worst["Sigma_bev vs reference"] = RC.err_rel(got["Sigmas_bev"][:, :m], gold["image/ref_Sigma_bev"])
    mu_bev = got["means_px"][:, :m] / vp.px_per_m + np.asarray(vp.origin_xy)
    assert RC.err_rel(mu_bev, gold["image/ref_mu_bev"]) <= 1e-12
    print("prep, worst difference / max:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= 1e-12, worst
    for v in range(3):  # the one-Gaussian drop-in, one row per view
        mu2, S2 = R.pushforward_gaussian_3d_to_2d(b["mu_world"][v], b["Sigma_world"][v], P[v], ctx=ctx)
        assert RC.err_rel(mu2, gold["image/ref_mu_bev"][v, v]) <= 1e-12
        assert RC.err_rel(S2, gold["image/ref_Sigma_bev"][v, v]) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("views", ["bev15", "single"])
def test_gpu_render_map_bev(ctx, restated, views):
    want = restated[views == "single"]
    vp, cfg, bcfg = _image_cfgs()
    kw = dict(fbm_seed=RC.IMAGE["fbm_seed"], fbm_modulate_scale=RC.IMAGE["fbm_modulate_scale"], ctx=ctx)
    batch = _host_batch(RC.build_image_batch())
    a = R.render_map_bev(batch, vp, cfg, bcfg, views, **kw)
    nv = len(want["images"])
    T = (RC.IMAGE["H"] // 32) * (RC.IMAGE["W"] // 32)
    assert a.images.shape == (nv, RC.IMAGE["H"], RC.IMAGE["W"], 3) and a.images.dtype == np.float64
    assert a.tile_counts.shape == (nv, T) and a.tile_indices.shape == (nv, T, RC.IMAGE["cap"])
    np.testing.assert_array_equal(a.tile_counts, np.stack(want["counts"]))
    np.testing.assert_array_equal(a.tile_indices, np.stack(want["indices"]))
    worst = RC.err(a.images, np.stack(want["images"]))
    print(views, "composed image, worst |difference|: %.3g" % worst)
    assert worst <= 1e-10
    assert a.images.min() >= 0.0 and a.images.max() <= 1.0 and a.images.max() > 0.05
    b = R.render_map_bev(batch, vp, cfg, bcfg, views, **kw)  # bit-reproducible from run to run
    assert a.images.tobytes() == b.images.tobytes() and a.tile_indices.tobytes() == b.tile_indices.tobytes()
    assert set(a.device) >= {"images", "tile_counts", "tile_indices", "means_px", "Sigmas_inv", "alphas", "colors", "fbm"}
    # a tile of the image is what the one-tile drop-in renders from the same 2D splats and list
    s = {k: a.device[k].download()[nv - 1] for k in ("means_px", "Sigmas_inv", "alphas", "colors")}
    t = T - 1
    oy, ox = (t // (RC.IMAGE["W"] // 32)) * 32, (t % (RC.IMAGE["W"] // 32)) * 32
    lst = a.tile_indices[nv - 1, t, :a.tile_counts[nv - 1, t]]
    one = R.render_tile_ewa((oy, ox), 32, s["means_px"], s["Sigmas_inv"], s["alphas"], s["colors"], lst, ctx=ctx)
    assert one.tobytes() == a.images[nv - 1, oy:oy + 32, ox:ox + 32].tobytes()
    np.testing.assert_array_equal(R.splat_indices_for_tile((oy, ox), 32, s["means_px"], s["Sigmas_inv"],
                                                           RC.IMAGE["cap"], ctx=ctx), lst)


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


FLOATS = ("mu_world", "Sigma_world", "eta", "mass", "color")


@pytest.mark.gpu
@pytest.mark.parametrize("m_view", [32, 8])
def test_gpu_renderable_batch(ctx, m_view):
    from gcslam.association import extract_atlas_map_view
    tiles = RC.build_map()
    dm = _device_map(ctx, tiles)
    ids = sorted(tiles)
    want, _ = RC.expected_batch(tiles, ids, m_view)
    n = want["primitive_ids"].shape[0]
    assert n == (32 + 16 if m_view == 32 else 16) and len(set(want["last_supported_scan_seq"])) < n // 2
    view = extract_atlas_map_view(dm, ids, m_view, eps_lift=RC.EPS_LIFT)
    dev = R.renderable_batch_from_view(view, RC.EPS_LIFT)
    got = dev.download()
    assert dev.count == n and dev.capacity == 3 * m_view
    np.testing.assert_array_equal(got.primitive_ids, want["primitive_ids"])
    np.testing.assert_array_equal(got.last_supported_scan_seq, want["last_supported_scan_seq"])
    assert got.primitive_ids.dtype == np.int64
    worst = {k: RC.err_rel(getattr(got, k), want[k]) for k in FLOATS}
    worst["Lambda_world"] = RC.err_rel(got.Lambda_world, want["Lambda_world"])
    print("m_tile_view", m_view, "batch, worst difference / max:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst[k] for k in FLOATS) <= 1e-10, worst   # the view's own bar (solve and inverse on the device)
    assert worst["Lambda_world"] <= 1e-10, worst
    # the copied fields are the view's own rows, and Lambda_world is the inverse of the row it stands by
    hv = view.download()
    row = {int(p): i for i, p in enumerate(hv["primitive_ids"]) if hv["valid_mask"][i]}
    sel = [row[int(p)] for p in got.primitive_ids]
    for k, src in (("mu_world", "positions"), ("Sigma_world", "covariances"), ("eta", "etas"), ("mass", "weights"),
                   ("color", "colors")):
        assert getattr(got, k).tobytes() == hv[src][sel].tobytes(), k
    lam = np.linalg.inv(got.Sigma_world + RC.EPS_LIFT * np.eye(3))
    assert RC.err_rel(got.Lambda_world, lam) <= 1e-12
    for k, a in dev.arrays.items():  # rows from count on are zero
        assert not a.download()[n:].any(), k
    # publish_renderable is the same batch, from the map
    pub = R.publish_renderable(dm, max_primitives=None if m_view == 32 else m_view, eps_lift=RC.EPS_LIFT)
    again = pub.download()
    for k in FLOATS + ("Lambda_world", "primitive_ids", "last_supported_scan_seq"):
        assert getattr(again, k).tobytes() == getattr(got, k).tobytes(), k


@pytest.mark.gpu
def test_gpu_renderable_batch_empty_and_rendered(ctx):
    dm = _device_map(ctx, RC.build_map(empty=True))
    pub = R.publish_renderable(dm)
    assert pub.count == 0 and pub.capacity == 3 * RC.M_TILE
    host = pub.download()
    assert host.mu_world.shape == (0, 3) and host.eta.shape == (0, RC.L, 3) and host.primitive_ids.shape == (0,)
    assert R.publish_renderable(dm, tile_ids=[]).count == 0
    vp = R.Viewport((-4.0, -4.0), 8.0, 64, 64)
    out = R.render_map_bev(dm, vp, views="single")      # an empty map renders black
    assert out.images.shape == (1, 64, 64, 3) and not out.images.any() and not out.tile_counts.any()
    assert (out.tile_indices == -1).all()
    full = R.render_map_bev(_device_map(ctx, RC.build_map()), vp, R.SplatRenderingConfig(max_splats_per_tile=8))
    assert full.images.shape == (15, 64, 64, 3) and np.isfinite(full.images).all() and full.images.max() > 0.05
    assert full.tile_counts.max() <= 8 and full.tile_counts.max() > 0


@pytest.mark.gpu
def test_gpu_entry_argument_errors(ctx):
    """The C entries reject what the Python layer rejects, before any launch."""
    z = _abi.DeviceArray(ctx, (64,), np.float64)
    zi = _abi.DeviceArray(ctx, (64,), np.int32)
    st = R._SplatStruct(z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, None)

    def call(n=1, nv=1, H=32, W=32, ts=32, cap=4):
        _abi.call("gc_render_ewa_tiles", ctx.handle, nv, n, ctypes.byref(st), H, W, ts, cap, 25.0, 1e-12, z.ptr, zi.ptr,
                  zi.ptr, ctx=ctx)
    for kw in (dict(ts=0), dict(ts=33), dict(H=48), dict(W=40), dict(cap=0), dict(cap=257), dict(n=-1), dict(nv=0),
               dict(nv=33), dict(H=0)):
        with pytest.raises(ValueError):
            call(**kw)
    img = _abi.DeviceArray(ctx, (2, 8, 16, 3), np.float64)
    cnt, idx = _abi.DeviceArray(ctx, (2, 2), np.int32), _abi.DeviceArray(ctx, (2, 2, 4), np.int32)
    img.upload(np.ones(img.shape))
    cnt.upload(np.ones(cnt.shape, np.int32))
    _abi.call("gc_render_ewa_tiles", ctx.handle, 2, 0, None, 8, 16, 8, 4, 25.0, 1e-12, img.ptr, cnt.ptr, idx.ptr, ctx=ctx)
    assert not img.download().any() and not cnt.download().any() and (idx.download() == -1).all()  # n = 0
