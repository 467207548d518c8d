"""plan_tile_residency (gcslam/primitive_map.py): the residency policy of DevicePrimitiveMap.ensure_tiles,
a pure host function. Wanted keys that are resident stay; victims are the slabs whose key is not wanted,
least recently wanted first, ties by the lowest slab; incoming keys take the victims in the order they
are asked for; a stored key is loaded, any other created."""

import pytest

from gcslam.primitive_map import TileMove, plan_tile_residency


def test_all_hits_is_an_empty_plan():
    assert plan_tile_residency([10, 11, 12], [3, 1, 2], [12, 10], []) == []
    assert plan_tile_residency([10, 11, 12], [0, 0, 0], [], [99]) == []
    assert plan_tile_residency([10, 11, 12], [0, 0, 0], [10, 11, 12], [10]) == []


def test_lru_victim_and_its_tie_break():
    # slab 1 was wanted longest ago
    assert plan_tile_residency([10, 11, 12], [5, 2, 4], [20], []) == [TileMove(1, 11, 20, False)]
    # a wanted slab is never a victim, however old its stamp
    assert plan_tile_residency([10, 11, 12], [5, 2, 4], [11, 20], []) == [TileMove(2, 12, 20, False)]
    # equal stamps: the lowest slab first
    assert plan_tile_residency([10, 11, 12], [7, 7, 7], [20, 21], []) == \
        [TileMove(0, 10, 20, False), TileMove(1, 11, 21, False)]
    assert plan_tile_residency([10, 11, 12], [7, 3, 3], [20], []) == [TileMove(1, 11, 20, False)]


def test_incoming_keys_are_placed_in_the_order_asked():
    # victims in LRU order (slabs 2, 0, 1), incoming in the order of wanted_keys (32, 30, 31)
    plan = plan_tile_residency([10, 11, 12], [2, 3, 1], [32, 30, 31], [])
    assert plan == [TileMove(2, 12, 32, False), TileMove(0, 10, 30, False), TileMove(1, 11, 31, False)]
    # resident keys among the wanted ones take no victim and do not shift the order
    plan = plan_tile_residency([10, 11, 12, 13], [4, 1, 3, 2], [41, 12, 40], [])
    assert plan == [TileMove(1, 11, 41, False), TileMove(3, 13, 40, False)]


def test_load_when_stored_create_when_not():
    plan = plan_tile_residency([10, 11], [1, 2], [20, 21], [21, 99])
    assert plan == [TileMove(0, 10, 20, False), TileMove(1, 11, 21, True)]


def test_a_key_evicted_and_wanted_again_is_loaded():
    """A walk as ensure_tiles drives it: the plan is applied, the evicted key joins the store, the
    wanted slabs are stamped."""
    resident, last, stored, clock = [1, 2, 3], [0, 0, 0], set(), 0

    def want(keys):
        nonlocal clock
        plan = plan_tile_residency(resident, last, keys, stored)
        for mv in plan:
            stored.add(mv.evicted)
            stored.discard(mv.incoming)
            resident[mv.slab] = mv.incoming
        clock += 1
        for k in keys:
            last[resident.index(k)] = clock
        return plan

    assert want([1, 2, 3]) == []
    assert want([2, 3]) == []
    assert want([4]) == [TileMove(0, 1, 4, False)]        # key 1: stamped longest ago
    assert want([1]) == [TileMove(1, 2, 1, True)]         # back from the store, into the next LRU slab
    assert want([2, 5]) == [TileMove(2, 3, 2, True), TileMove(0, 4, 5, False)]
    assert stored == {3, 4} and resident == [5, 1, 2]


def test_too_many_keys_raises():
    with pytest.raises(ValueError, match="slabs"):
        plan_tile_residency([10, 11], [0, 0], [1, 2, 3], [])
    with pytest.raises(ValueError, match="slabs"):
        plan_tile_residency([10, 11], [0, 0], [10, 11, 3], [])


def test_duplicate_keys_raise():
    with pytest.raises(ValueError, match="duplicate"):
        plan_tile_residency([10, 11, 12], [0, 0, 0], [20, 20], [])
    with pytest.raises(ValueError, match="duplicate"):
        plan_tile_residency([10, 10, 12], [0, 0, 0], [20], [])
    with pytest.raises(ValueError, match="stamps"):
        plan_tile_residency([10, 11, 12], [0, 0], [20], [])
