"""The batched maintenance's test cases and host pieces, without a GPU: the margins that make each
case's discrete outcomes well determined (mapmaint_cases.expected, from the oracle loop alone), what
each case must cover, and the argument errors of primitive_map_maintain and of
primitive_map_update_from_association(maintenance="device"), all raised before any device call."""

import numpy as np
import pytest

import mapmaint_cases as MM
import mapupdate_cases as MC

# measured margins (cull, max_primitives cut, merge threshold, merge order):
#   kat      1.0e+03, none,    1.0e+00, 1.0e+00
#   tiny_m1  5.0e+02, none,    none,    none
#   tiny_m2  5.0e+02, none,    1.0e+00, none
#   ragged   1.2e-02, none,    2.1e-04, 3.6e-07
#   topk     9.4e-03, 1.3e-03, 3.7e-04, 1.9e-07
#   cap      1.1e-01, none,    none,    none
#   wide     2.5e-02, none,    1.4e+00, none


@pytest.mark.parametrize("name", MM.CASES)
def test_case_margins(name):
    ref = MM.expected(MM.build(name))
    for k, v in ref["margin"].items():
        assert v >= 1e-9, (k, v)


def test_cases_are_the_issue_s():
    k = MM.build("kat")
    assert (len(k["tiles"]), k["m_tile"], k["active"]) == (1, 3, [0])
    assert (MM.config(k)["primitive_merge_threshold"], MM.config(k)["k_merge_pairs_tile"],
            MM.config(k)["max_tile_size"]) == (0.5, 1, 10)
    r = MM.build("ragged")
    assert (len(r["tiles"]), r["m_tile"], r["P"], r["active"]) == (5, 300, 44850, [3, 0, 4])
    c = MM.config(r)
    assert (c["primitive_cull_weight_threshold"], c["primitive_forgetting_factor"], c["primitive_merge_threshold"],
            c["k_merge_pairs_tile"]) == (1e-3, 0.995, 2.0, 16)
    assert r["m_tile"] > 256  # more than one block per tile
    valid = [int(t["valid_mask"].sum()) for t in r["tiles"]]
    assert 0.6 * 300 < valid[0] < 0.8 * 300 and valid[3] == 0 and valid[4] == 1
    t = MM.build("topk")
    assert t["active"] == [0, 1, 2, 3] and t["max_primitives"] == 150
    assert all(np.array_equal(a[f], b[f]) for a, b in zip(t["tiles"], r["tiles"]) for f in a)  # the ragged map
    w = MM.build("wide")
    assert (len(w["tiles"]), w["m_tile"], len(w["active"]), len(set(w["active"]))) == (70, 8, 64, 64)
    assert all(int(t["valid_mask"].sum()) == 6 for t in w["tiles"]) and w["cfg"] == {}


def test_kat_is_the_known_answer():
    ref = MM.expected(MM.build("kat"))
    (row,), (t,) = ref["rows"], ref["tiles"]
    assert (row["n_culled"], row["n_merged"], row["state"]) == (0, 1, "ran")
    assert list(t["valid_mask"]) == [True, False, True]
    assert np.isclose(t["weights"][0], 2.0 * 0.995) and t["weights"][1] == 0.0


def test_tiny_covers_no_pair_and_one_pair():
    one, two = MM.build("tiny_m1"), MM.build("tiny_m2")
    assert (one["m_tile"], one["P"], two["m_tile"], two["P"]) == (1, 0, 2, 1)
    for c in (one, two):
        assert len(c["tiles"]) == 2 and c["active"] == [0, 1] and all(t["valid_mask"].all() for t in c["tiles"])
    assert [r["state"] for r in MM.expected(one)["rows"]] == ["noop", "noop"]
    assert [(r["state"], r["n_merged"]) for r in MM.expected(two)["rows"]] == [("ran", 1), ("ran", 1)]


def test_ragged_covers_cull_merge_and_the_untouched_tiles():
    case = MM.build("ragged")
    ref = MM.expected(case)
    by_tile = dict(zip(case["active"], ref["rows"]))
    assert by_tile[0]["n_merged"] >= 8 and by_tile[0]["n_culled"] >= 1 and by_tile[0]["state"] == "ran"
    assert by_tile[3]["state"] == "noop" and by_tile[3]["n_valid"] == 0
    assert by_tile[4]["state"] == "noop" and by_tile[4]["n_valid"] == 1 and by_tile[4]["n_culled"] == 0
    for d in (1, 2):  # inactive: the very arrays of the input
        assert all(ref["tiles"][d][f] is case["tiles"][d][f] for f in case["tiles"][d])


def test_topk_takes_and_skips_the_branch():
    ref = MM.expected(MM.build("topk"))
    assert [r["topk"] for r in ref["rows"]] == [True, True, False, False]
    assert all(abs(r["n_valid"] - 210) <= 10 for r in ref["rows"][:2])
    assert 0.3 * 300 < ref["rows"][2]["n_valid"] < 0.5 * 300 and ref["rows"][3]["n_valid"] == 0
    # the reference keeps max_primitives + 1: the threshold is the (max_primitives + 1)-th largest, culled below it
    assert all(r["n_valid"] - r["n_culled"] == 151 for r in ref["rows"][:2])


def test_cap_merges_nothing_and_still_culls():
    case = MM.build("cap")
    ref = MM.expected(case)
    assert MM.config(case)["max_tile_size"] == 20 and case["m_tile"] == 40
    assert [r["state"] for r in ref["rows"]] == ["capped", "noop", "noop"]
    assert [r["n_valid"] for r in ref["rows"]] == [40, 1, 0] and all(r["n_merged"] == 0 for r in ref["rows"])
    assert ref["rows"][0]["n_culled"] >= 1
    for d in case["active"]:
        np.testing.assert_array_equal(ref["tiles"][d]["weights"], 0.995 * case["tiles"][d]["weights"])


# ----------------------------------------------------------------------------- argument errors
class _HostMap:
    """The attributes the operators read before their first device call (as test_mapupdate._HostMap)."""
    ctx = None
    n_lobes = 3

    def __init__(self, n_tiles, m_tile, ptrs=("valid_mask", "cam_mass")):
        self.tile_keys, self.m_tile, self.n_tiles = list(range(n_tiles)), m_tile, n_tiles
        self.ptrs = {k: 1 for k in ptrs}

    def dense_tile(self, key):
        return self.tile_keys.index(int(key)) if int(key) in self.tile_keys else -1


def test_maintain_argument_errors_raise_before_any_device_call():
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_maintain
    m = _HostMap(4, 64)
    bad = [
        dict(tile_ids=[0, 1, 0]),                                       # duplicate ids
        dict(tile_ids=[0, 4]),                                          # not a tile of the map
        dict(tile_ids=[-1]),
        dict(tile_ids=[0], atlas_map=_HostMap(4, 64, ptrs=("cam_mass",))),  # no maintenance fields
        dict(tile_ids=[0], atlas_map=_HostMap(2, 65537), config=MapUpdateConfig(max_tile_size=0)),  # merge would run
    ]
    for kw in bad:
        kw = dict(dict(atlas_map=m), **kw)
        with pytest.raises(ValueError):
            primitive_map_maintain(**kw)


def test_maintain_of_no_tiles_touches_nothing():
    from gcslam.primitive_map import primitive_map_maintain
    m = _HostMap(4, 64)  # has no context: any device call would fail
    res, cert, eff = primitive_map_maintain(m, [])
    assert (res.n_culled_total, res.mass_dropped_total, res.n_merged_total, res.tile_certs) == (0, 0.0, 0, [])
    assert res.n_culled.shape == res.mass_dropped.shape == res.n_merged.shape == (0,)
    assert cert.exact and (eff.objective_name, eff.predicted, eff.realized) == ("primitive_map_maintain", 0.0, 0.0)
    # over the cap the 65536 rule does not apply (nothing would merge); the empty list still returns
    primitive_map_maintain(_HostMap(2, 70000), [])


def test_update_device_mode_argument_errors():
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_update_from_association

    class _Obj:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class _KeyMap(_HostMap):
        def __init__(self, keys, m_tile, **kw):
            super().__init__(len(keys), m_tile, **kw)
            self.tile_keys = list(keys)

    case = MC.build("blocks")

    def call(maintenance, atlas_map=None, active=None):
        return primitive_map_update_from_association(
            atlas_map or _KeyMap(case["ids"], case["m_tile"]), _Obj(**case["assoc"]), _Obj(**case["meas"]),
            case["active"] if active is None else active, case["pose"], MC.TIMESTAMP, MC.SCAN_SEQ,
            MapUpdateConfig(**case["cfg"]), maintenance=maintenance)

    with pytest.raises(ValueError, match="maintenance"):
        call("host")
    with pytest.raises(ValueError):
        call("device", active=case["active"] + case["active"][:1])
    with pytest.raises(ValueError):
        call("device", atlas_map=_KeyMap(case["ids"], case["m_tile"], ptrs=("cam_mass",)))
