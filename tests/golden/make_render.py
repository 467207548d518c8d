"""TEST INFRASTRUCTURE — records the reference's own outputs for the rendering cases into
tests/golden/render.npz.

The renderer and the BEV pushforward are pure NumPy in the reference (backend/rendering.py,
common/bev_pushforward.py) and import without JAX. This script loads those two files in place (the
reference tree exists only in the build container; its packages' __init__ files pull in ROS and JAX,
so the two files are loaded by path), runs

    splat_indices_for_tile, render_tile_ewa, fbm_at_splat_positions,
    opacity_from_logdet, vmf_shading_multi_lobe,
    pushforward_gaussian_3d_to_2d, oblique_P_from_config, oblique_Ps_bev15

on the inputs of tests/render_cases.py and stores the inputs and the returned values, with the
fields and defaults of the two configuration classes, so the GPU box reads the npz. Nothing here
computes anything of its own.

    python tests/golden/make_render.py REFERENCE_ROOT
"""

from __future__ import annotations

import dataclasses
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import render_cases as RC  # noqa: E402


def _load(ref_root, rel, name):
    path = os.path.join(ref_root, "fl_ws", "src", "fl_slam_poc", "fl_slam_poc", rel)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    R = _load(ref_root, os.path.join("backend", "rendering.py"), "ref_rendering")
    B = _load(ref_root, os.path.join("common", "bev_pushforward.py"), "ref_bev_pushforward")
    assert "jax" not in sys.modules
    out = {}
    for name in RC.TILE_CASES:
        c = RC.build_tile(name)
        pre = "tile/" + name + "/"
        for k in ("means", "Sigmas_inv", "alphas", "colors") + (("world_xy",) if name == RC.FBM_TILE_CASE else ()):
            out[pre + k] = c[k]
        idx = R.splat_indices_for_tile(c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["cap"], 1e-12)
        out[pre + "ref_indices"] = idx
        args = (c["origin"], c["tile_size"], c["means"], c["Sigmas_inv"], c["alphas"], c["colors"])
        out[pre + "ref_image"] = R.render_tile_ewa(*args, splat_indices=idx)
        if name.endswith("_n5"):
            out[pre + "ref_image_empty"] = R.render_tile_ewa(*args, splat_indices=np.array([], np.int64))
        if name in RC.NONE_LIST:
            out[pre + "ref_image_none"] = R.render_tile_ewa(*args, splat_indices=None)
        if name == RC.FBM_TILE_CASE:
            f = RC.FBM_TILE
            out[pre + "ref_image_fbm"] = R.render_tile_ewa(*args, splat_indices=idx, means_world_xy=c["world_xy"],
                                                           fbm_octaves=f["octaves"], fbm_gain=f["gain"],
                                                           fbm_seed=f["seed"], fbm_modulate_scale=f["scale"])
    xy = RC.build_fbm()
    out["fbm/xy"] = xy
    for octaves, seed in RC.FBM_RUNS:
        out[f"fbm/ref_o{octaves}_s{seed}"] = R.fbm_at_splat_positions(xy, octaves=octaves, gain=RC.FBM_GAIN, seed=seed)
    b = RC.build_image_batch()
    m = RC.PREP_ROWS
    for k, v in b.items():
        out["image/" + k] = v[:m]  # the rows the reference's pieces are recorded on
    mus, Sigs, shades = [], [], []
    for P, vd in RC.image_views():
        pf = [B.pushforward_gaussian_3d_to_2d(b["mu_world"][i], b["Sigma_world"][i], P) for i in range(m)]
        mus.append(np.array([p[0] for p in pf]))
        Sigs.append(np.array([p[1] for p in pf]))
        shades.append(np.array([R.vmf_shading_multi_lobe(vd, *RC.shading_inputs(b, i)) for i in range(m)]))
    out["image/ref_mu_bev"], out["image/ref_Sigma_bev"] = np.array(mus), np.array(Sigs)
    out["image/ref_shading"] = np.array(shades)
    out["opacity/logdet"] = RC.LOGDETS
    out["opacity/ref_default"] = np.array([R.opacity_from_logdet(float(x)) for x in RC.LOGDETS])
    out["opacity/ref_other"] = np.array([R.opacity_from_logdet(float(x), **RC.OPACITY_OTHER) for x in RC.LOGDETS])
    out["views/ref_Ps_default"] = B.oblique_Ps_bev15(B.BEVPushforwardConfig())
    out["views/ref_P_default"] = B.oblique_P_from_config(B.BEVPushforwardConfig())
    icfg = B.BEVPushforwardConfig(oblique_phi_deg=RC.IMAGE["oblique_phi_deg"], n_views=RC.IMAGE["n_views"],
                                  phi_center_deg=RC.IMAGE["phi_center_deg"], phi_span_deg=RC.IMAGE["phi_span_deg"])
    out["views/ref_Ps_image"] = B.oblique_Ps_bev15(icfg)
    out["views/ref_Ps_one"] = B.oblique_Ps_bev15(B.BEVPushforwardConfig(n_views=1))
    defaults = {cls.__name__: dataclasses.asdict(cls()) for cls in (R.SplatRenderingConfig, B.BEVPushforwardConfig)}
    out["config/defaults_json"] = np.frombuffer(json.dumps(defaults, sort_keys=True).encode(), np.uint8)
    dst = os.path.join(HERE, "render.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
