"""Tile residency of DevicePrimitiveMap on the device: the tile image entries
(gc_primitive_map_tile_export / _import / _reset, gc_maptiles.hip) and ensure_tiles. Images and
reloaded tiles are compared bit for bit: nothing here computes, every byte is moved."""

import ctypes as C
import time

import numpy as np
import pytest

from oracle import gc_oracle as O
from test_map_ops import _random_tile

L = 3
_COLOUR = ("cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom", "rgb", "colors")


def _random_map(ctx, n_tiles, m_tile, seed, packed=True, colours=True):
    """A map of random tiles (every field non-trivial, rgb and colors included) and its host fields."""
    from gcslam.primitive_map import DevicePrimitiveMap
    rng = np.random.default_rng(seed)
    tiles = []
    for _ in range(n_tiles):
        t = _random_tile(rng, m_tile, 0.6)
        t["rgb"] = rng.uniform(0, 1, (m_tile, 3))
        t["colors"] = rng.uniform(0, 1, (m_tile, 3))
        tiles.append(t)
    full = {k: np.concatenate([t[k] for t in tiles]) for k in tiles[0] if colours or k not in _COLOUR}
    full["valid_mask"] = full["valid_mask"].astype(np.uint8)
    dm = DevicePrimitiveMap(n_tiles, m_tile, n_lobes=L, track_colors=colours, ctx=ctx, packed=packed)
    dm.upload(**full)
    return dm


def _bits(fields):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in fields.items()}


def _tile_call(dm, name, tile, image=None):
    from gcslam import _abi
    s0, n = dm.tile_range(tile)
    args = [dm.ctx.handle, C.byref(dm.struct()), s0, n] + ([] if image is None else [image.ctypes.data])
    _abi.call(name, *args, ctx=dm.ctx)


def _image(dm):
    return np.full(dm.m_tile * dm.image_slot_bytes, 0xA5, np.uint8)


def _assert_empty(fields, m_tile):
    ref = O.empty_tile(m_tile, L)
    for k, v in fields.items():
        want = ref[k].astype(np.uint8) if k == "valid_mask" else ref[k]
        assert np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(want).tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("colours", [True, False])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("m_tile", [5, 300])
def test_gpu_tile_image_round_trip(ctx, m_tile, packed, colours):
    """export -> reset -> import on the middle tile of three: reset leaves create_empty_tile, import
    restores every field bit for bit, and the other two tiles never change."""
    dm = _random_map(ctx, 3, m_tile, 10 + m_tile, packed, colours)
    assert ("rgb" in dm.ptrs) == colours
    before = dm.download()
    img = _image(dm)
    _tile_call(dm, "gc_primitive_map_tile_export", 1, img)
    _tile_call(dm, "gc_primitive_map_tile_reset", 1)
    ctx.sync()
    after_reset = dm.download()
    s = slice(m_tile, 2 * m_tile)
    _assert_empty({k: v[s] for k, v in after_reset.items()}, m_tile)
    for k in before:
        for o in (slice(0, m_tile), slice(2 * m_tile, 3 * m_tile)):
            assert after_reset[k][o].tobytes() == before[k][o].tobytes(), k
    # the image holds the tile's fields where the record layout puts them; absent fields as the empty tile
    got = _bits(dm.image_fields(img))
    assert got == _bits({k: v[s] for k, v in before.items()})
    if not colours:
        rec = img.reshape(m_tile, dm.image_slot_bytes)
        o = int(dm._image_off[11])  # rgb
        assert rec[:, o:o + 24].copy().view(np.float64).tobytes() == np.full((m_tile, 3), 0.5).tobytes()
        o = int(dm._image_off[7])   # cam_mass
        assert not rec[:, o:o + 8].any()
    _tile_call(dm, "gc_primitive_map_tile_import", 1, img)
    ctx.sync()
    assert _bits(dm.download()) == _bits(before)


@pytest.mark.gpu
@pytest.mark.parametrize("m_tile", [5, 300])
def test_gpu_tile_image_crosses_layouts(ctx, m_tile):
    """An image exported from a packed map and imported into a per-field map gives equal fields, and
    back; a map without colour fields takes what it holds and ignores the rest."""
    src = _random_map(ctx, 2, m_tile, 3, packed=True)
    dst = _random_map(ctx, 2, m_tile, 4, packed=False)
    nocol = _random_map(ctx, 2, m_tile, 5, packed=False, colours=False)
    want, keep = src.download_tile(1), dst.download_tile(1)
    img = _image(src)
    _tile_call(src, "gc_primitive_map_tile_export", 1, img)
    ctx.sync()
    _tile_call(dst, "gc_primitive_map_tile_import", 0, img)
    _tile_call(nocol, "gc_primitive_map_tile_import", 0, img)
    ctx.sync()
    assert _bits(dst.download_tile(0)) == _bits(want)
    assert _bits(dst.download_tile(1)) == _bits(keep)
    assert _bits(nocol.download_tile(0)) == _bits({k: v for k, v in want.items() if k not in _COLOUR})
    back = _image(dst)
    _tile_call(dst, "gc_primitive_map_tile_export", 0, back)
    ctx.sync()
    assert _bits(src.image_fields(back)) == _bits(want)


@pytest.mark.gpu
def test_gpu_tile_entries_check_their_range(ctx):
    dm = _random_map(ctx, 2, 5, 1)
    from gcslam import _abi
    img = _image(dm)
    for s0, n in ((6, 5), (-1, 5), (0, 11)):
        with pytest.raises(ValueError, match="tile range"):
            _abi.call("gc_primitive_map_tile_export", ctx.handle, C.byref(dm.struct()), s0, n, img.ctypes.data, ctx=ctx)
        with pytest.raises(ValueError, match="tile range"):
            _abi.call("gc_primitive_map_tile_reset", ctx.handle, C.byref(dm.struct()), s0, n, ctx=ctx)
    with pytest.raises(ValueError, match="NULL"):
        _abi.call("gc_primitive_map_tile_import", ctx.handle, C.byref(dm.struct()), 0, 5, None, ctx=ctx)


def _walk_map(ctx):
    dm = _random_map(ctx, 3, 8, 21)
    A, B, Cc = 101, 102, 103
    dm.set_tile_keys([A, B, Cc])
    dm.tile_count = {0: 5, 1: 6, 2: 7}
    dm.total_count = 18
    dm._tile_cc = [True, False, True]
    return dm, (A, B, Cc, 104)


@pytest.mark.gpu
def test_gpu_ensure_tiles_all_hits_does_not_wait(ctx):
    """Behind a 0.5 s device spin an all-hit call returns at once: it launches nothing and waits for
    nothing (a call that waited for the stream would take the spin's time)."""
    from gcslam import _abi
    dm, (A, B, Cc, D) = _walk_map(ctx)
    before = dm.download()
    ctx.sync()
    _abi.call("gc_test_device_spin", ctx.handle, 0.5, ctx=ctx)
    t0 = time.perf_counter()
    r = dm.ensure_tiles([Cc, A])
    t1 = time.perf_counter()
    ctx.sync()
    t2 = time.perf_counter()
    print(f"all-hit ensure_tiles {t1 - t0:.5f} s, synchronise {t2 - t1:.4f} s")
    assert t1 - t0 < 0.25, t1 - t0
    assert (r.hits, r.loaded, r.created, r.evicted, r.dense) == ([Cc, A], [], [], [], [2, 0])
    assert dm.stored_keys() == [] and dm.tile_keys == [A, B, Cc]
    assert _bits(dm.download()) == _bits(before)


@pytest.mark.gpu
def test_gpu_ensure_tiles_walk_evicts_and_reloads(ctx):
    """Keys A B C, then D (evicts A, the least recently wanted), then A again: loaded back bit for bit
    with its tile_count and colour flag, into the slab B leaves."""
    dm, (A, B, Cc, D) = _walk_map(ctx)
    tiles = {k: dm.download_tile(d) for d, k in enumerate(dm.tile_keys)}
    r = dm.ensure_tiles([A, B, Cc])
    assert (r.hits, r.evicted, r.dense) == ([A, B, Cc], [], [0, 1, 2])
    dm.ensure_tiles([B, Cc])
    r = dm.ensure_tiles([D])
    assert (r.hits, r.loaded, r.created, r.evicted, r.dense) == ([], [], [D], [A], [0])
    assert dm.tile_keys == [D, B, Cc] and dm.stored_keys() == [A]
    assert dm.tile_count == {1: 6, 2: 7} and dm._tile_cc == [False, False, True]
    assert dm.total_count == 18 and dm.key_count(A) == 5
    _assert_empty(dm.download_tile(0), 8)
    assert _bits(dm.key_fields(A)) == _bits(tiles[A])      # from the store
    assert _bits(dm.download_tile(1)) == _bits(tiles[B]) and _bits(dm.download_tile(2)) == _bits(tiles[Cc])
    r = dm.ensure_tiles([A])
    assert (r.hits, r.loaded, r.created, r.evicted, r.dense) == ([], [A], [], [B], [1])
    assert dm.tile_keys == [D, A, Cc] and dm.stored_keys() == [B]
    assert dm.tile_count == {1: 5, 2: 7} and dm._tile_cc == [False, True, True]
    assert _bits(dm.download_tile(1)) == _bits(tiles[A])
    assert _bits(dm.key_fields(B)) == _bits(tiles[B]) and dm.key_count(B) == 6
    assert _bits(dm.download_tile(2)) == _bits(tiles[Cc])
    with pytest.raises(ValueError, match="slabs"):
        dm.ensure_tiles([1, 2, 3, 4])
    with pytest.raises(ValueError, match="host store"):
        dm.set_tile_keys([B, 7, 8])


@pytest.mark.gpu
def test_gpu_ensure_tiles_raises_with_a_pipeline_attached(ctx):
    from oracle import cases
    from test_gpu_configs import _pipeline
    dm, (A, B, Cc, D) = _walk_map(ctx)
    case = cases.build(H=2, n_az=256, n_scans=1, io="computed")
    pipe = _pipeline(case, ctx, 2, case["n"], True)
    pipe.attach_primitive_map(dm, 0.2)
    with pytest.raises(RuntimeError, match="attached"):
        dm.ensure_tiles([A])  # even an all-hit call
    pipe.attach_primitive_map(None)
    assert dm.ensure_tiles([D]).created == [D]
    pipe.close()
