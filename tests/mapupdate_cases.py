"""Inputs of the map-update tests, built on the CPU alone (the pattern of vpe_cases.py): a hex-tiled
map, the oracle's view and OT association of a measurement batch with it, the active stencil, and
z_t. The unmodified association gives novelty = 0 on every row (all scores tie), so a seeded third
of the valid rows has its row mass lowered by a factor in [0, 0.9] after the association, as
vpe_cases.py edits a responsibility row (the factors are scaled by a / row_mass, see build).

The seeds are picked so that the discrete outputs are well determined (check_margins): every valid
row's world mean lies >= 1e-9 tile widths from a tile boundary on all three axes, consecutive
eviction keys among the first k_insert + 1 of each tile differ by >= 1e-9 relative, and every cull
and merge decision is >= 1e-9 relative from its threshold. test_mapupdate.py asserts them, and what
each case must cover, without a GPU."""

import numpy as np

from oracle import gc_oracle as O
from test_association import _hex_map, _meas

import mapupdate_restatement as MR

L = 3
H_TILE = 2.0
TIMESTAMP, SCAN_SEQ, NEXT_ID = 12.5, 14, 1000

_GRID5 = [(a, b, 0) for a in range(-2, 3) for b in range(-2, 3)]


def _stencil(radius_z):
    """ma_hex_stencil_tile_ids order around cell (0, 0, 0): increasing cz, then the sorted radius-1 disk."""
    return [(dq, dr, dz) for dz in range(-radius_z, radius_z + 1) for dq, dr in O.hex_disk_axial(1)]


#            N, K, map cells, active cells, m_tile, n_valid (slots filled), view size, k_insert, block, seed, yaw_only
CASES = {
    "smallest": (1, 1, [(0, 0, 0)], [(0, 0, 0)], 8, 6, 8, 1, 256, 1, False),
    "ragged": (300, 8, _GRID5, _stencil(0), 64, 58, 32, 16, 256, 0, False),
    "placeholder": (300, 8, _GRID5 + [(dq, dr, dz) for dq, dr, dz in _stencil(1) if dz != 0], _stencil(1), 64, 58, 32,
                    16, 256, 1, True),
    "blocks": (70, 8, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], 64,
               58, 32, 8, 32, 2, False),
}
_cache = {}


def build(name, seed=None):
    """dict(tiles, ids, active, m_tile, view, meas, assoc, pose, cfg, ...) — computed once per case and
    shared; callers must not modify it."""
    key = (name, seed)
    if key in _cache:
        return _cache[key]
    N, K, cells, act_cells, m_tile, n_valid, m_view, k_ins, block, seed0, yaw_only = CASES[name]
    rng = np.random.default_rng(seed0 if seed is None else seed)
    tiles = _hex_map(rng, m_tile, n_valid, cells)
    for (c1, c2, cz) in cells:  # the cz != 0 tiles of the placeholder stencil start empty
        if cz != 0:
            tiles[int(O.tile_ids_from_cells(c1, c2, cz))] = O.empty_tile(m_tile, L)
    ids = list(tiles)
    active = [int(O.tile_ids_from_cells(*c)) for c in act_cells]
    view = O.extract_atlas_map_view(tiles, ids, m_view, m_tile)
    if name == "smallest":
        meas = _meas(rng, N, 0.5, 1.5)
        meas["valid_mask"][:] = True
    elif name == "blocks":
        meas = _meas(rng, N, 0.0, 4.0)
    else:
        meas = _meas(rng, N)
    meas["colors"] = rng.uniform(-0.1, 1.1, (N, 3))  # some outside [0, 1]: the clip
    meas["sources"] = (rng.uniform(0, 1, N) < 0.6).astype(np.int32)  # both sources
    res, _ = O.associate_primitives_ot(meas, view, dict(k_assoc=K, scan_seq=SCAN_SEQ, h_tile=H_TILE))
    assoc = {k: np.array(res[k]) for k in ("responsibilities", "candidate_pool_indices", "candidate_tile_ids",
                                           "candidate_slots", "row_masses", "cost_matrix")}
    vi = np.flatnonzero(meas["valid_mask"])
    low = vi[rng.uniform(0, 1, vi.shape[0]) < 1.0 / 3.0] if name != "smallest" else vi
    # factors in [0, 0.9], drawn as 0.9 u a / row_mass: the unbalanced OT's row masses are 40-200 x the uniform
    # marginal a here, so a factor uniform in [0, 0.9] would leave novelty = max(a - row_mass, 0) at 0 on nearly
    # every row; these leave row_mass = 0.9 u a, novelty = a (1 - 0.9 u) > 0 on the lowered third
    a = 1.0 / max(vi.shape[0], 1)
    factor = 0.9 * rng.uniform(0.0, 1.0, low.shape[0]) * np.minimum(a / assoc["row_masses"][low], 1.0)
    assert np.all((factor >= 0.0) & (factor <= 0.9))
    assoc["row_masses"][low] *= factor
    pose = np.zeros(6)
    pose[:2] = rng.normal(size=2) * 0.1
    if yaw_only:  # z stays in [0, 2): the cz = -1 and cz = +1 tiles receive no measurement
        pose[5] = 0.07
    else:
        pose[2] = 0.02
        pose[3:] = rng.normal(size=3) * 0.03
    cfg = dict(k_insert_tile=k_ins, block_size=block, h_tile=H_TILE)
    out = dict(name=name, tiles=tiles, ids=ids, active=active, m_tile=m_tile, m_view=m_view, view=view, meas=meas,
               assoc=assoc, pose=pose, cfg=cfg, N=N, K=K, k_ins=k_ins)
    _cache[key] = out
    return out


def reference(case, maintenance=True):
    """The restatement's result for a case (computed once per maintenance flag; do not modify)."""
    key = "ref_m" if maintenance else "ref"
    if key not in case:
        case[key] = MR.map_update(case["tiles"], case["assoc"], case["meas"], case["active"], case["pose"], TIMESTAMP,
                                  SCAN_SEQ, case["cfg"], NEXT_ID, maintenance)
    return case[key]


def check_margins(ref):
    assert ref["margin_tile"] >= 1e-9, ref["margin_tile"]
    assert ref["margin_evict"] >= 1e-9, ref["margin_evict"]
    assert ref["margin_cull"] >= 1e-9, ref["margin_cull"]
    assert ref["margin_merge"] >= 1e-9, ref["margin_merge"]
