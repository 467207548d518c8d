"""The map update's test cases and host pieces, without a GPU: what each case of mapupdate_cases.py
must cover and the margins that make its discrete outputs well determined (taken from the
restatement's own intermediates, tests/mapupdate_restatement.py), the argument errors of
primitive_map_update_from_association (all raised before anything touches the device), and
gcslam.tiling against the oracle's tiling helpers."""

import numpy as np
import pytest

from oracle import gc_oracle as O

import mapupdate_cases as MC

# seed -> measured margins (tile boundary, eviction keys, cull, merge), maintenance on:
#   smallest    1: 3.1e-01, none (no finite pair), 2.8e+03, 3.7e-01
#   ragged      0: 5.8e-04, 4.0e-03, 4.2e-01, 7.9e-04
#   placeholder 1: 4.5e-05, 3.4e-03, 7.7e-01, 1.2e-03
#   blocks      2: 7.6e-04, none, 1.0e+00, 3.1e-03


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_margins_and_shapes(name):
    case = MC.build(name)
    for maintenance in (False, True):
        ref = MC.reference(case, maintenance)
        MC.check_margins(ref)
        A, k = len(case["active"]), case["k_ins"]
        for f in ("insert_indices", "insert_valid", "insert_target_slots", "new_ids"):
            assert ref[f].shape == (A, k), f
        assert len(set(case["active"])) == A and all(t in case["tiles"] for t in case["active"])
        ids = ref["new_ids"][ref["insert_valid"]]
        assert np.array_equal(ids, MC.NEXT_ID + np.arange(ids.shape[0]))  # ids run on across tiles
        assert ref["next_global_id"] == MC.NEXT_ID + ref["n_inserted"] == MC.NEXT_ID + ids.shape[0]


def test_case_shapes_are_the_issue_s():
    s = MC.build("smallest")
    assert (s["N"], s["K"], len(s["active"]), s["m_tile"], s["k_ins"]) == (1, 1, 1, 8, 1)
    r = MC.build("ragged")
    assert (r["N"], r["K"], len(r["active"]), len(r["ids"]), r["m_tile"], r["k_ins"]) == (300, 8, 7, 25, 64, 16)
    assert r["cfg"]["block_size"] == 256 and r["N"] == 256 + 44  # the second block is padded
    assert not r["meas"]["valid_mask"].all() and set(np.unique(r["meas"]["sources"])) == {0, 1}
    occupied = [int(t["valid_mask"].sum()) for t in r["tiles"].values()]
    assert max(occupied) + r["k_ins"] > r["m_tile"]  # k_insert evicts live slots
    p = MC.build("placeholder")
    assert len(p["active"]) == 21 and p["active"][7:14] == r["active"]
    b = MC.build("blocks")
    assert (b["N"], b["cfg"]["block_size"]) == (70, 32)


def test_ragged_covers_the_ranking_paths():
    case = MC.build("ragged")
    ref = MC.reference(case)
    nov, valid = ref["novelty"], case["meas"]["valid_mask"]
    rich = False
    for a, t in enumerate(case["active"]):
        it = ref["meas_tile_ids"] == t
        if it.sum() > case["k_ins"] and (nov[it] > 0).sum() >= 4 and ((nov[it] == 0) & valid[it]).sum() >= 4:
            rich = True
            chosen = ref["insert_indices"][a]
            assert (nov[chosen] == 0).any() and (nov[chosen] > 0).any()  # the tie-break decides the tail
    assert rich
    assert ref["chosen_invalid"] >= 1   # an in-tile invalid row is chosen (inserted with zero mass)
    assert ref["evicted_valid"] >= 1    # an eviction hits a valid slot
    assert (~np.isin(case["assoc"]["candidate_tile_ids"], case["active"])).any()  # a candidate names an inactive tile
    assert not any(ref["placeholder"])


def test_placeholder_covers_the_empty_and_short_tiles():
    case = MC.build("placeholder")
    ref = MC.reference(case)
    ph = np.asarray(ref["placeholder"])
    assert ph[:7].all() and ph[14:].all() and not ph[7:14].any()  # the cz = -1 and cz = +1 tiles
    assert all(ref["in_tile_counts"][a] == 0 for a in np.flatnonzero(ph))
    assert ref["insert_valid"][ph].all()  # the all-ones mask
    assert np.array_equal(ref["insert_indices"][0], np.arange(case["k_ins"]))  # all tied at -1e30: lowest rows
    assert any(0 < n < case["k_ins"] for n in ref["in_tile_counts"])  # fewer in-tile rows than k_insert
    assert ref["chosen_invalid"] >= 1 and ref["evicted_valid"] >= 1


def test_blocks_spans_three_blocks():
    case = MC.build("blocks")
    ref = MC.reference(case, False)
    N, bs = case["N"], case["cfg"]["block_size"]
    slots = case["assoc"]["candidate_slots"]
    per_block = [np.unique(slots[b * bs:min((b + 1) * bs, N)]).shape[0] for b in range(3)]
    assert ref["n_fused"] == len(case["active"]) * sum(per_block)
    # the stamp reaches slots no row of the tile fused into: every named slot number, in every active tile
    named = np.unique(slots)
    own = 0
    for t in case["active"]:
        assert np.all(ref["tiles"][t]["timestamps"][named] == MC.TIMESTAMP)
        own += np.setdiff1d(named, slots[case["assoc"]["candidate_tile_ids"] == t]).shape[0]
    assert own > 0  # some of them named only by rows of other tiles


# ----------------------------------------------------------------------------- argument errors
class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _HostMap:
    """The attributes the operator reads before its first device call."""
    ctx = None
    n_lobes = 3
    ptrs = {"valid_mask": 1, "cam_mass": 1}

    def __init__(self, keys, m_tile):
        self.tile_keys, self.m_tile = list(keys), m_tile

    def dense_tile(self, key):
        return self.tile_keys.index(int(key)) if int(key) in self.tile_keys else -1


def _call(case, **over):
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_update_from_association
    kw = dict(atlas_map=_HostMap(case["ids"], case["m_tile"]), assoc=_Obj(**case["assoc"]), batch=_Obj(**case["meas"]),
              active=case["active"], pose=case["pose"], cfg=MapUpdateConfig(**case["cfg"]))
    kw.update(over)
    return primitive_map_update_from_association(kw["atlas_map"], kw["assoc"], kw["batch"], kw["active"], kw["pose"],
                                                 MC.TIMESTAMP, MC.SCAN_SEQ, kw["cfg"])


def test_argument_errors_raise_before_any_launch():
    from gcslam.primitive_map import (GC_MAP_UPDATE_MAX_ACTIVE, GC_MAP_UPDATE_MAX_INSERT, GC_MAP_UPDATE_MAX_ROWS,
                                      MapUpdateConfig)
    from gcslam.constants import GC_N_FEAT, GC_N_SURFEL
    assert GC_MAP_UPDATE_MAX_ROWS >= GC_N_FEAT + GC_N_SURFEL
    case = MC.build("blocks")
    cfg = case["cfg"]
    missing = int(O.tile_ids_from_cells(40, 40, 0))
    bad = [
        dict(active=case["active"] + [missing]),                                  # a key the map does not hold
        dict(active=case["active"] + case["active"][:1]),                         # duplicate keys
        dict(cfg=MapUpdateConfig(**dict(cfg, k_insert_tile=0))),
        dict(cfg=MapUpdateConfig(**dict(cfg, k_insert_tile=case["m_tile"] + 1))),  # > m_tile
        dict(cfg=MapUpdateConfig(**dict(cfg, k_insert_tile=case["N"] + 1)),
             atlas_map=_HostMap(case["ids"], 128)),                                # > N
        dict(assoc=_Obj(**dict(case["assoc"], candidate_slots=case["assoc"]["candidate_slots"][:, :4]))),  # K
        dict(assoc=_Obj(**dict(case["assoc"], row_masses=case["assoc"]["row_masses"][:-1]))),              # N
        dict(batch=_Obj(**dict(case["meas"], weights=case["meas"]["weights"][:-1]))),                      # N
        dict(batch=_Obj(**dict(case["meas"], etas=case["meas"]["etas"][:, :2]))),                          # lobes
        dict(pose=np.array([0.0, np.nan, 0.0, 0.0, 0.0, 0.0])),
        dict(pose=np.array([0.0, 0.0, 0.0, np.inf, 0.0, 0.0])),
        dict(pose=np.zeros(5)),
        dict(cfg=MapUpdateConfig(**dict(cfg, h_tile=0.0))),
        dict(cfg=MapUpdateConfig(**dict(cfg, h_tile=-2.0))),
        dict(cfg=MapUpdateConfig(**dict(cfg, block_size=0))),
    ]
    for over in bad:
        with pytest.raises(ValueError):
            _call(case, **over)
    # beyond the plan's LDS bounds: rows, proposals, active tiles
    N = GC_MAP_UPDATE_MAX_ROWS + 1
    big_assoc = _Obj(responsibilities=np.zeros((N, 2)), candidate_tile_ids=np.zeros((N, 2), np.int64),
                     candidate_slots=np.zeros((N, 2), np.int64), row_masses=np.zeros(N))
    big_batch = _Obj(Lambdas=np.zeros((N, 3, 3)), thetas=np.zeros((N, 3)), etas=np.zeros((N, 3, 3)),
                     weights=np.zeros(N), valid_mask=np.zeros(N, bool), colors=np.zeros((N, 3)),
                     sources=np.zeros(N, np.int32))
    with pytest.raises(ValueError, match="bounds"):
        _call(case, assoc=big_assoc, batch=big_batch)
    n = GC_MAP_UPDATE_MAX_INSERT + 8
    mid_assoc = _Obj(**{k: getattr(big_assoc, k)[:n] for k in big_assoc.__dict__})
    mid_batch = _Obj(**{k: getattr(big_batch, k)[:n] for k in big_batch.__dict__})
    with pytest.raises(ValueError, match="bounds"):
        _call(case, assoc=mid_assoc, batch=mid_batch, atlas_map=_HostMap(case["ids"], 4096),
              cfg=MapUpdateConfig(**dict(cfg, k_insert_tile=GC_MAP_UPDATE_MAX_INSERT + 1)))
    many = list(range(GC_MAP_UPDATE_MAX_ACTIVE + 1))
    with pytest.raises(ValueError, match="bounds"):
        _call(case, atlas_map=_HostMap(many, case["m_tile"]), active=many)


# ----------------------------------------------------------------------------- gcslam.tiling
def test_tiling_matches_oracle():
    from gcslam import tiling as T
    for r in (0, 1, 2, 3):
        assert T.hex_disk_axial(r) == O.hex_disk_axial(r)
    assert len(T.hex_disk_axial(1)) == 7 and len(T.hex_disk_axial(2)) == 19
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-50.0, 50.0, (500, 3))  # negative coordinates: floor, not truncation
    xyz[:6] = [[-0.5, 0.1, -0.1], [-2.0, 0.0, 0.0], [1.999999, -3.0, 2.0], [0.0, 0.0, 0.0], [-1e-9, -1e-9, -1e-9],
               [3.0, -2.0 * 3.0 / np.sqrt(3.0), 5.0]]
    for h in (2.0, 0.7):
        c1, c2, cz = O.tile_cells_from_xyz(xyz, h)
        cells = T.tile_cells_from_xyz_batch(xyz, h)
        assert np.array_equal(cells, np.stack([c1, c2, cz], axis=1))
        ids = T.tile_ids_from_xyz_batch(xyz, h)
        assert ids.dtype == np.int64 and np.array_equal(ids, O.tile_ids_from_cells(c1, c2, cz))
        assert np.array_equal(T.tile_ids_from_cells(c1, c2, cz), O.tile_ids_from_cells(c1, c2, cz))
    assert (cells[:, 0] < 0).any() and (cells[:, 1] < 0).any() and (cells[:, 2] < 0).any()
    assert T.tile_id_from_cell_3d(-1, 2, -3) == int(O.tile_ids_from_cells(-1, 2, -3))


def test_stencil_order_and_counts():
    from gcslam import tiling as T
    center = np.array([-0.3, 4.1, -2.5])
    c1, c2, cz = (int(v[0]) for v in O.tile_cells_from_xyz(center[None], 2.0))
    for rxy, rz, n in ((1, 0, 7), (2, 0, 19), (1, 1, 21), (2, 1, 57)):
        ids = T.ma_hex_stencil_tile_ids(center, 2.0, rxy, rz)
        want = [int(O.tile_ids_from_cells(c1 + dq, c2 + dr, cz + dz)) for dz in range(-rz, rz + 1)
                for dq, dr in O.hex_disk_axial(rxy)]
        assert ids == want and len(ids) == n == len(set(ids))
    # the cases' active lists are this stencil around the origin cell
    assert MC.build("ragged")["active"] == T.ma_hex_stencil_tile_ids(np.array([0.5, 0.5, 0.5]), 2.0, 1, 0)
    assert MC.build("placeholder")["active"] == T.ma_hex_stencil_tile_ids(np.array([0.5, 0.5, 0.5]), 2.0, 1, 1)
