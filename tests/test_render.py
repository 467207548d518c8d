"""Rendering without a GPU: the fixture recorded from the reference's own NumPy code
(tests/golden/render.npz, tests/golden/make_render.py), the conditions under which its cases pin a
device implementation, the restatement (tests/render_restatement.py) held to the recorded outputs at
1e-12, and the Python layer's argument checks, configuration defaults and view matrices.

The worst restatement-vs-reference differences are printed by test_restatement_matches_reference
and recorded in DESIGN.md §4 (Rendering)."""

import dataclasses
import json

import numpy as np
import pytest

import render_cases as RC
import render_restatement as RS
from gcslam import _abi
from gcslam import rendering as R

BAR = 1e-12
TILES = list(RC.TILE_CASES)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(RC.GOLDEN))


@pytest.fixture(scope="module")
def image():
    return RC.restated_image()


def _tile(gold, name):
    pre = "tile/" + name + "/"
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", TILES)
def test_fixture_holds_the_tile_cases(gold, name):
    built, g = RC.build_tile(name), _tile(gold, name)
    for k in ("means", "Sigmas_inv", "alphas", "colors"):
        assert g[k].tobytes() == built[k].tobytes(), k
    assert g["ref_indices"].dtype == np.int64 and g["ref_image"].shape == (built["tile_size"],) * 2 + (3,)
    assert ("ref_image_none" in g) == (name in RC.NONE_LIST)


def test_fixture_holds_the_other_cases(gold):
    assert gold["fbm/xy"].tobytes() == RC.build_fbm().tobytes()
    b = RC.build_image_batch()
    for k, v in b.items():
        assert gold["image/" + k].tobytes() == v[:RC.PREP_ROWS].tobytes(), k
    assert gold["opacity/logdet"].tobytes() == RC.LOGDETS.tobytes()


def _cond2(S):
    ev = np.linalg.eigvalsh(S)
    return float((ev[:, -1] / ev[:, 0]).max()) if S.shape[0] else 1.0


@pytest.mark.parametrize("name", TILES)
def test_tile_conditions(name):
    """Every bbox comparison has a margin >= 1e-9 px; consecutive dist_sq of the survivors, one past the
    cap included, differ by >= 1e-9 relative, except the deliberate exact tie; cond(Sigma_inv) <= 100."""
    c = RC.build_tile(name)
    idx, cd = RS.tile_bins(c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["cap"])
    assert cd["margin"] >= 1e-9 and cd["gap"] >= 1e-9, cd
    assert cd["ties"] == (1 if name == "special" else 0)
    assert _cond2(c["Sigmas_inv"]) <= 100.0
    if name.startswith("cap"):
        assert cd["survivors"] == 200 > c["cap"] == len(idx)  # the cap cuts
    if name == "special":
        assert 0 not in idx                                   # wholly outside
        pos = {int(i): p for p, i in enumerate(idx)}
        assert pos[7] == pos[3] + 1                           # the exact tie: the lower index first
        d = np.array([c["origin"][1] + 0.5, c["origin"][0] + 0.5]) - c["means"][5]
        assert 0.5 * d @ c["Sigmas_inv"][5] @ d > 25.0 and 5 in idx  # -q / 2 below the log_clip floor


def test_image_conditions(image):
    b = RC.build_image_batch()
    ev = np.linalg.eigvalsh(b["Sigma_world"])
    assert (ev[:, -1] / ev[:, 0]).max() <= 100.0
    for v, cd in enumerate(image["cond"]):
        assert cd["margin"] >= 1e-9 and cd["gap"] >= 1e-9 and cd["ties"] == 0, (v, cd)
        assert cd["cut"] >= 1, "no tile of the image case reaches the cap"
        assert _cond2(image["splats"][v]["Sigmas_inv"]) <= 100.0
    assert image["counts"][0].min() >= 1 and RC.IMAGE["H"] != RC.IMAGE["W"]
    assert len({im.tobytes() for im in image["images"]}) == RC.IMAGE["n_views"]  # the views differ


def test_fbm_conditions():
    xy = RC.build_fbm()
    m = RS.fbm_integer_margin(xy, 5)
    assert m[RC.FBM_EXACT, 0] == 0.0
    m[RC.FBM_EXACT, 0] = np.inf
    assert m.min() >= 1e-9
    assert (xy < 0).any() and (xy > 0).any() and (np.abs(xy) > 990).sum() >= 16
    assert RS.fbm_integer_margin(RC.build_image_batch()["mu_world"][:, :2], RC.RENDER_CFG["fbm_octaves"]).min() >= 1e-9
    assert RS.fbm_integer_margin(RC.build_tile(RC.FBM_TILE_CASE)["world_xy"], RC.FBM_TILE["octaves"]).min() >= 1e-9
    assert float(np.abs(xy).max()) * 2.0 ** 4 < 2.0 ** 31  # the integer hash's domain


def test_restatement_matches_reference(gold):
    worst = {}

    def hold(key, got, want, rel=False):
        e = RC.err_rel(got, want) if rel else RC.err(got, want)
        worst[key] = max(worst.get(key, 0.0), e)

    for name in TILES:
        c, g = RC.build_tile(name), _tile(gold, name)
        idx, _ = RS.tile_bins(c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["cap"])
        np.testing.assert_array_equal(idx, g["ref_indices"])
        args = (c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["alphas"], c["colors"])
        hold("tile image", RS.render_tile(*args, idx), g["ref_image"])
        if "ref_image_none" in g:
            hold("tile image", RS.render_tile(*args, None), g["ref_image_none"])
        if "ref_image_empty" in g:
            assert not g["ref_image_empty"].any() and not RS.render_tile(*args, np.zeros(0, np.int64)).any()
        if "ref_image_fbm" in g:
            f = RC.FBM_TILE
            mod = (1.0 - f["scale"]) + f["scale"] * RS.fbm(c["world_xy"], f["octaves"], f["gain"], f["seed"])
            hold("tile image", RS.render_tile(*args[:5], c["colors"] * mod[:, None], idx), g["ref_image_fbm"])
    for octaves, seed in RC.FBM_RUNS:
        hold("fbm", RS.fbm(gold["fbm/xy"], octaves, RC.FBM_GAIN, seed), gold[f"fbm/ref_o{octaves}_s{seed}"])
    b, m = RC.build_image_batch(), RC.PREP_ROWS
    for v, (P, vd) in enumerate(RC.image_views()):
        mu_bev, S_bev = RS.pushforward(b["mu_world"][:m], b["Sigma_world"][:m], P)
        hold("mu_bev", mu_bev, gold["image/ref_mu_bev"][v], rel=True)
        hold("Sigma_bev", S_bev, gold["image/ref_Sigma_bev"][v], rel=True)
        hold("shading", RS.vmf_shading(vd, b["eta"][:m]), gold["image/ref_shading"][v], rel=True)
    hold("opacity", RS.opacity_from_logdet(RC.LOGDETS), gold["opacity/ref_default"], rel=True)
    o = RC.OPACITY_OTHER
    hold("opacity", RS.opacity_from_logdet(RC.LOGDETS, o["gamma"], o["logdet0"], o["alpha_min"]),
         gold["opacity/ref_other"], rel=True)
    print("restatement vs reference, worst difference:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= BAR, worst


def test_view_matrices_and_directions(gold):
    np.testing.assert_array_equal(R.oblique_Ps_bev15(R.BEVPushforwardConfig()), gold["views/ref_Ps_default"])
    np.testing.assert_array_equal(R.oblique_P_from_config(R.BEVPushforwardConfig()), gold["views/ref_P_default"])
    np.testing.assert_array_equal(R.oblique_Ps_bev15(R.BEVPushforwardConfig(n_views=1)), gold["views/ref_Ps_one"])
    icfg = R.BEVPushforwardConfig(oblique_phi_deg=RC.IMAGE["oblique_phi_deg"], n_views=RC.IMAGE["n_views"],
                                  phi_center_deg=RC.IMAGE["phi_center_deg"], phi_span_deg=RC.IMAGE["phi_span_deg"])
    np.testing.assert_array_equal(R.oblique_Ps_bev15(icfg), gold["views/ref_Ps_image"])
    for views in ("bev15", "single"):
        P, vd = R.bev_views(icfg, views)
        assert P.shape == ((3 if views == "bev15" else 1), 2, 3) and vd.shape == P.shape[:1] + (3,)
        assert np.abs(np.einsum("vij,vj->vi", P, vd)).max() <= 1e-15  # the null vector of P
        np.testing.assert_allclose(np.linalg.norm(vd, axis=1), 1.0, atol=1e-15)
    for (P, vd), (P2, vd2) in zip(RC.image_views(), zip(*R.bev_views(icfg, "bev15"))):
        assert P.tobytes() == P2.tobytes() and vd.tobytes() == vd2.tobytes()


def test_config_defaults_are_the_references(gold):
    ref = json.loads(bytes(gold["config/defaults_json"]).decode())
    assert dataclasses.asdict(R.SplatRenderingConfig()) == ref["SplatRenderingConfig"]
    assert dataclasses.asdict(R.BEVPushforwardConfig()) == ref["BEVPushforwardConfig"]
    with pytest.raises(Exception):
        R.SplatRenderingConfig().tile_size = 8  # frozen, as in the reference
    assert [f.name for f in dataclasses.fields(R.RenderablePrimitiveBatch)][:7] == [
        "mu_world", "Sigma_world", "Lambda_world", "eta", "mass", "color", "primitive_ids"]


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_abi, "lib", boom)
    monkeypatch.setattr(_abi, "default_context", boom)
    monkeypatch.setattr(_abi, "call", boom)


def test_argument_errors_need_no_library(monkeypatch):
    _no_device(monkeypatch)
    b = RC.build_image_batch()
    batch = R.RenderablePrimitiveBatch(mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None,
                                       eta=b["eta"], mass=b["mass"], color=b["color"])
    C, V = R.SplatRenderingConfig, R.Viewport
    ok = V((0.0, 0.0), 8.0, 64, 96)
    for cfg, vp in ((C(tile_size=0), ok), (C(tile_size=33), ok), (C(tile_size=2.5), ok),
                    (C(), V((0.0, 0.0), 8.0, 65, 96)), (C(), V((0.0, 0.0), 8.0, 64, 100)),
                    (C(tile_size=24), V((0.0, 0.0), 8.0, 48, 64)), (C(), V((0.0, 0.0), 8.0, 0, 96)),
                    (C(max_splats_per_tile=0), ok), (C(max_splats_per_tile=257), ok),
                    (C(), V((0.0, 0.0), 0.0, 64, 96)), (C(), V((float("nan"), 0.0), 8.0, 64, 96)),
                    (C(fbm_octaves=33), ok), (C(eps=float("inf")), ok)):
        with pytest.raises(ValueError):
            R.render_map_bev(batch, vp, cfg)
    for kw in (dict(views="bev16"), dict(fbm_seed=-1), dict(fbm_seed=1 << 31), dict(fbm_modulate_scale=float("nan")),
               dict(bev_cfg=R.BEVPushforwardConfig(n_views=33))):
        with pytest.raises(ValueError):
            R.render_map_bev(batch, ok, **kw)
    with pytest.raises(ValueError):
        R.render_map_bev(object(), ok)
    with pytest.raises(ValueError):
        R._check_raster_args(32, 64, 96, 64, -1)  # a negative n
    with pytest.raises(ValueError):
        R.fbm_at_splat_positions(np.array([[2.0 ** 28, 0.0]]), octaves=5)  # outside the hash's domain
    for kw in (dict(octaves=-1), dict(octaves=33), dict(seed=-1), dict(gain=float("nan"))):
        with pytest.raises(ValueError):
            R.fbm_at_splat_positions(np.zeros((2, 2)), **kw)
    c = RC.build_tile("t8_n5")
    args = (c["origin"], 8, c["means"], c["Sigmas_inv"], c["alphas"], c["colors"])
    with pytest.raises(IndexError):
        R.render_tile_ewa(*args, splat_indices=np.array([5]))
    with pytest.raises(ValueError):
        R.render_tile_ewa((1 << 25, 0), *args[1:])
    with pytest.raises(ValueError):
        R.splat_indices_for_tile((0, -(1 << 25)), 8, c["means"], c["Sigmas_inv"])


def test_empty_inputs_need_no_library(monkeypatch):
    """rendering.py:269-270, :324-327: no splats, or an empty index list."""
    _no_device(monkeypatch)
    z2, z22 = np.zeros((0, 2)), np.zeros((0, 2, 2))
    idx = R.splat_indices_for_tile((0, 0), 32, z2, z22)
    assert idx.shape == (0,) and idx.dtype == np.int64
    assert not R.render_tile_ewa((0, 0), 40, z2, z22, np.zeros(0), np.zeros((0, 3))).any()  # clamped to 32
    c = RC.build_tile("t8_n5")
    out = R.render_tile_ewa(c["origin"], 8, c["means"], c["Sigmas_inv"], c["alphas"], c["colors"],
                            splat_indices=np.array([], np.int64))
    assert out.shape == (8, 8, 3) and not out.any()
    assert R.fbm_at_splat_positions(z2).shape == (0,)
