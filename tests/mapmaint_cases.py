"""Inputs of the batched-maintenance tests, built on the CPU alone (the pattern of mapupdate_cases.py):
maps of dense tiles, the active list, the step-12b parameters, and the expected outcome from the
oracle's per-tile operators looped over the active tiles in order, cull -> forget -> merge-reduce
with the tile-size cap rule of mapupdate_restatement.map_update.

The seeds are picked so that every discrete outcome is well determined (expected() measures, and
test_mapmaint.py asserts): every valid weight >= 1e-9 relative from the cull threshold, the weights
around a max_primitives cut distinct by >= 1e-9 relative, every valid pair distance >= 1e-9 relative
from the merge threshold, and the distances below the threshold with the first one above pairwise
>= 1e-9 relative apart (the greedy selection's order is then not a rounding question)."""

import numpy as np

from oracle import gc_oracle as O
from test_map_ops import _merge_kat_tile, _random_tile

import mapupdate_restatement as MR

L = 3
_FIELDS = tuple(O.empty_tile(1, L))


def _one_valid(rng, M):
    t = _random_tile(rng, M, 1.0)
    t["valid_mask"] = np.zeros(M, bool)
    t["valid_mask"][int(np.argmax(t["weights"]))] = True  # it survives every cull threshold used here
    return t


def _ragged_map():
    rng = np.random.default_rng(7)
    M = 300
    tiles = [_random_tile(rng, M, 0.7), _random_tile(rng, M, 0.7), _random_tile(rng, M, 0.4), O.empty_tile(M, L),
             _one_valid(rng, M)]
    return tiles, M


def _tiny(m_tile):
    """Two fully valid tiles of m_tile slots; at m_tile = 2 each tile's pair is 1 cm apart."""
    tiles = []
    for d in range(2):
        t = O.empty_tile(m_tile, L)
        t["Lambdas"][:] = np.eye(3) * (1.0 + 0.25 * d)
        t["thetas"][:] = t["Lambdas"] @ np.array([0.3 * d, 0.0, 0.0])
        if m_tile == 2:
            t["thetas"][1] = t["Lambdas"][1] @ np.array([0.3 * d + 0.01, 0.0, 0.0])
        t["weights"][:] = [0.5 + 0.125 * d, 0.75][:m_tile]
        t["primitive_ids"][:] = np.arange(m_tile) + 10 * d
        t["valid_mask"][:] = True
        t["lidar_mass"][:] = t["weights"]
        tiles.append(t)
    return tiles


def _wide_map():
    rng = np.random.default_rng(11)
    tiles = []
    for _ in range(70):
        t = _random_tile(rng, 8, 1.0)
        t["valid_mask"] = np.zeros(8, bool)
        t["valid_mask"][rng.permutation(8)[:6]] = True
        tiles.append(t)
    return tiles, [int(d) for d in rng.permutation(70)[:64]]


_BASE = dict(primitive_cull_weight_threshold=1e-3, primitive_forgetting_factor=0.995)


def _spec(name):
    """(tiles in dense order, m_tile, active dense tiles, MapUpdateConfig fields, max_primitives)"""
    if name == "kat":
        return [_merge_kat_tile()], 3, [0], dict(_BASE, primitive_merge_threshold=0.5, k_merge_pairs_tile=1,
                                                  max_tile_size=10), None
    if name in ("tiny_m1", "tiny_m2"):
        m = 1 if name == "tiny_m1" else 2
        return _tiny(m), m, [0, 1], dict(_BASE, primitive_merge_threshold=0.5, k_merge_pairs_tile=4), None
    if name in ("ragged", "topk"):
        tiles, M = _ragged_map()
        cfg = dict(_BASE, primitive_merge_threshold=2.0, k_merge_pairs_tile=16)
        return (tiles, M, [3, 0, 4], cfg, None) if name == "ragged" else (tiles, M, [0, 1, 2, 3], cfg, 150)
    if name == "cap":
        rng = np.random.default_rng(3)
        tiles = [_random_tile(rng, 40, 1.0), _one_valid(rng, 40), O.empty_tile(40, L)]
        return tiles, 40, [0, 1, 2], dict(_BASE, primitive_merge_threshold=2.0, k_merge_pairs_tile=16,
                                           max_tile_size=20), None
    if name == "wide":
        tiles, active = _wide_map()
        return tiles, 8, active, {}, None  # the defaults of MapUpdateConfig
    raise KeyError(name)


CASES = ("kat", "tiny_m1", "tiny_m2", "ragged", "topk", "cap", "wide")
_cache = {}


def build(name):
    """dict(tiles, m_tile, active, cfg, max_primitives, P) — computed once per case and shared; callers
    must not modify it."""
    if name not in _cache:
        tiles, m_tile, active, cfg, maxp = _spec(name)
        for t in tiles:
            assert set(t) == set(_FIELDS) and t["weights"].shape == (m_tile,)
        _cache[name] = dict(name=name, tiles=tiles, m_tile=m_tile, active=active, cfg=cfg, max_primitives=maxp,
                            P=m_tile * (m_tile - 1) // 2)
    return _cache[name]


def config(case):
    """All step-12b parameters of the case (the oracle's defaults where the case sets none)."""
    return dict(MR.DEFAULTS, **case["cfg"])


def flat(case):
    """The map's fields as flat (n_tiles * m_tile, ...) arrays, as DevicePrimitiveMap.upload takes them."""
    full = {k: np.concatenate([t[k] for t in case["tiles"]]) for k in _FIELDS}
    full["valid_mask"] = full["valid_mask"].astype(np.uint8)
    return full


def _min_gap(x):
    x = np.sort(np.asarray(x, np.float64))
    if x.shape[0] < 2:
        return np.inf
    return float(np.min((x[1:] - x[:-1]) / np.maximum(np.maximum(np.abs(x[1:]), np.abs(x[:-1])), 1e-300)))


def expected(case):
    """The oracle loop over the active tiles (computed once; do not modify): the tiles after, per
    active tile n_culled / mass_dropped / sum_w / n_valid / n_merged / topk / merge state, and the
    margins."""
    if "ref" in case:
        return case["ref"]
    c = config(case)
    thr, mt, maxp = c["primitive_cull_weight_threshold"], c["primitive_merge_threshold"], case["max_primitives"]
    tiles = list(case["tiles"])
    rows = []
    margin = dict(cull=np.inf, topk=np.inf, merge_thr=np.inf, merge_order=np.inf)
    for d in case["active"]:
        t = tiles[d]
        M = case["m_tile"]
        vm = np.asarray(t["valid_mask"], bool)
        w = t["weights"]
        row = dict(n_valid=int(vm.sum()), sum_w=float(np.sum(w)), topk=False)
        if vm.any():
            margin["cull"] = min(margin["cull"], float(np.min(np.abs(w[vm] - thr)) / thr))
        n_below = int(np.sum(vm & (w < thr)))
        if maxp is not None and row["n_valid"] - n_below > maxp and maxp < M:
            row["topk"] = True
            sw = np.sort(w * vm)[::-1]
            margin["topk"] = min(margin["topk"], _min_gap(sw[max(maxp - 1, 0):maxp + 2]))
        t, row["n_culled"], row["mass_dropped"] = O.primitive_map_cull(t, thr, maxp)
        t = O.primitive_map_forget(t, c["primitive_forgetting_factor"])
        nv = int(np.sum(t["valid_mask"]))
        capped = int(c["max_tile_size"]) > 0 and M > int(c["max_tile_size"])
        noop = M < 2 or nv < 2 or int(c["k_merge_pairs_tile"]) <= 0
        row["state"] = "noop" if noop else ("capped" if capped else "ran")
        row["n_merged"] = 0
        if not capped:  # mapupdate_restatement.map_update: the budget cap (:1881-1890)
            if not noop:
                dist = MR._merge_distances(t, c["eps_lift"])
                dist = dist[np.isfinite(dist)]
                if dist.size:
                    margin["merge_thr"] = min(margin["merge_thr"], float(np.min(np.abs(dist - mt)) / mt))
                    s = np.sort(dist)
                    margin["merge_order"] = min(margin["merge_order"], _min_gap(s[:int(np.sum(s < mt)) + 1]))
            t, row["n_merged"] = O.primitive_map_merge_reduce(t, mt, int(c["k_merge_pairs_tile"]), c["eps_psd"],
                                                              c["eps_lift"])
        row["n_after"] = int(np.sum(t["valid_mask"]))
        tiles[d] = t
        rows.append(row)
    case["ref"] = dict(tiles=tiles, rows=rows, margin=margin)
    return case["ref"]
