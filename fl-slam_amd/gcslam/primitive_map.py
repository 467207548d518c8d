"""Device-resident PrimitiveMap and its operators (backend/structures/primitive_map.py):
primitive_map_fuse (:992-1163) with the world pushforward of transform_gaussian_to_world
(backend/pipeline.py:1248-1256) fused in (the C5 map update), and the maintenance operators
primitive_map_insert_masked (:807-982), primitive_map_cull (:1175-1305), primitive_map_forget
(:1314-1390), primitive_map_recency_inflate (:1400-1490) and primitive_map_merge_reduce
(:1809-2030); primitive_map_update_from_association chains them as the post-pose map update of
backend/pipeline.py:1232-1492 does (step 12b), fuse and novelty insert in one device pass, and
primitive_map_maintain runs its cull / forget / merge-reduce over all active tiles in another. The map
lives in HBM as one flat array of n_tiles * m_tile slots (tile t, local slot j -> t * m_tile + j);
every operator runs in place on its tile. The AtlasMap bookkeeping (next_global_id, total_count,
per-tile count) stays on the host, as in the reference."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._abi import (GC_MAP_MAINTAIN_STATS_TILE, GC_MAP_UPDATE_MAX_ACTIVE, GC_MAP_UPDATE_MAX_INSERT, GC_MAP_UPDATE_MAX_K,
                   GC_MAP_UPDATE_MAX_ROWS, GC_MAP_UPDATE_STATS_HEAD, GC_MAP_UPDATE_STATS_TILE)
from .certificates import CertBundle, ExpectedEffect, InfluenceCert, MapUpdateCert
from .constants import (GC_ASSOC_BLOCK_SIZE, GC_CHART_ID, GC_EPS_LIFT, GC_EPS_MASS, GC_EPS_PSD, GC_H_TILE,
                        GC_K_INSERT_TILE, GC_K_MERGE_PAIRS_PER_TILE, GC_PRIMITIVE_CULL_WEIGHT_THRESHOLD,
                        GC_PRIMITIVE_FORGETTING_FACTOR, GC_PRIMITIVE_MERGE_MAX_TILE_SIZE,
                        GC_PRIMITIVE_MERGE_THRESHOLD, GC_RECENCY_DECAY_LAMBDA, GC_RECENCY_MIN_SCALE)

GC_VMF_N_LOBES = 3

_F64 = ("Lambdas", "thetas", "etas", "weights", "timestamps")
_I64 = ("last_supported_scan_seq", "last_update_scan_seq")
_COL = ("cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom", "rgb", "colors")
_MAINT = ("valid_mask", "created_timestamps", "primitive_ids")


_MapStruct = _abi.STRUCTS["gc_primitive_map"]  # its pointers are _F64 + _I64 + _COL + _MAINT, in that order
_InsertStruct = _abi.STRUCTS["gc_insert_batch"]
_FuseStruct = _abi.STRUCTS["gc_fuse_batch"]


class TileMove(NamedTuple):
    """One slab of a residency plan: the key that leaves it, the key that comes in, and whether that key
    is loaded from the host store (else it is created empty)."""
    slab: int
    evicted: int
    incoming: int
    load: bool


def plan_tile_residency(resident_keys: Sequence[int], last_used: Sequence[int], wanted_keys: Sequence[int],
                        stored_keys: Iterable[int]) -> List[TileMove]:
    """Which slabs change so that every wanted key is resident (host only, no device). Wanted keys that
    are resident stay where they are. Victims are the slabs whose key is not wanted, least recently
    wanted first (last_used[slab]: the stamp of the last call that wanted the slab's key), ties by the
    lowest slab. Incoming keys take the victims in the order of wanted_keys; a key in stored_keys is
    loaded, any other is created empty. ValueError for duplicate keys or more wanted keys than slabs."""
    resident = [int(k) for k in resident_keys]
    wanted = [int(k) for k in wanted_keys]
    stored = {int(k) for k in stored_keys}
    if len(last_used) != len(resident):
        raise ValueError(f"{len(last_used)} use stamps for {len(resident)} slabs")
    if len(set(wanted)) != len(wanted):
        raise ValueError(f"duplicate tile keys in {wanted}")
    if len(set(resident)) != len(resident):
        raise ValueError(f"duplicate resident tile keys in {resident}")
    if len(wanted) > len(resident):
        raise ValueError(f"{len(wanted)} tiles wanted, the map holds {len(resident)} slabs")
    want = set(wanted)
    here = set(resident)
    victims = sorted((d for d, k in enumerate(resident) if k not in want), key=lambda d: (int(last_used[d]), d))
    incoming = [k for k in wanted if k not in here]
    return [TileMove(d, resident[d], k, k in stored) for d, k in zip(victims, incoming)]


@dataclass
class TileResidency:
    """What DevicePrimitiveMap.ensure_tiles did: the keys found resident, loaded from the host store,
    created empty and evicted to the store, and the dense tile of every requested key, in request order."""
    hits: List[int]
    loaded: List[int]
    created: List[int]
    evicted: List[int]
    dense: List[int]


@dataclass
class _StoredTile:
    """A tile that is not resident: its image (gc_primitive_map_tile_export), its count in the AtlasMap
    bookkeeping (None: never recorded) and whether its colours were the fuse's estimate."""
    image: np.ndarray
    tile_count: Optional[int]
    colors_current: bool


class DevicePrimitiveMap:
    """n_tiles x m_tile slots of PrimitiveMapTile fields (create_empty_tile, primitive_map.py:148-175).

    packed=True (default) keeps one record per slot in HBM (gc_primitive_map_record_layout: the
    fuse's read-modify-write fields in the record's first two 128-B lines); upload / download
    transpose to and from the reference's per-field arrays on the device (gc_copy_strided).
    packed=False keeps the per-field arrays themselves.

    The n_tiles slabs hold the tiles named by tile_keys. ensure_tiles brings other keys in, as the
    reference's AtlasMap creates tiles on demand (primitive_map.py:183-211): the tile that has to leave
    a slab goes to a host store owned by the map (its image, tile_count and colour flag) and comes back
    from there when it is wanted again. next_global_id and total_count cover resident and stored tiles."""

    def __init__(self, n_tiles: int, m_tile: int, n_lobes: int = GC_VMF_N_LOBES, track_colors: bool = True,
                 ctx=None, packed: bool = True):
        self.ctx = ctx or _abi.default_context()
        self.n_tiles, self.m_tile, self.n_lobes = int(n_tiles), int(m_tile), int(n_lobes)
        M = self.M = self.n_tiles * self.m_tile
        self.shapes = dict(Lambdas=(M, 3, 3), thetas=(M, 3), etas=(M, n_lobes, 3), weights=(M,), timestamps=(M,),
                           last_supported_scan_seq=(M,), last_update_scan_seq=(M,), cam_mass=(M,), lidar_mass=(M,),
                           rgb_cam_accum=(M, 3), rgb_cam_denom=(M,), rgb=(M, 3), colors=(M, 3),
                           valid_mask=(M,), created_timestamps=(M,), primitive_ids=(M,))
        self.dtypes = {k: np.dtype(np.float64) for k in self.shapes}
        self.dtypes.update(last_supported_scan_seq=np.dtype(np.int64), last_update_scan_seq=np.dtype(np.int64),
                           primitive_ids=np.dtype(np.int64), valid_mask=np.dtype(np.uint8))
        names = [k for k in _F64 + _I64 + _COL + _MAINT if track_colors or k not in _COL]
        self.packed = bool(packed)
        self.ptrs: Dict[str, int] = {}
        self.fields: Dict[str, _abi.DeviceArray] = {}  # per-field arrays (packed=False)
        off = np.zeros(16, np.int64)
        sb = C.c_int64(0)
        _abi.call("gc_primitive_map_record_layout", self.n_lobes, off.ctypes.data, C.byref(sb))
        self.image_slot_bytes = int(sb.value)  # one slot of a tile image, whatever the map's layout
        self._image_off = off.copy()
        if self.packed:
            self.slot_bytes = int(sb.value)
            self.records = _abi.DeviceArray(self.ctx, M * self.slot_bytes, np.uint8)
            self.records.zero()
            order = _F64 + _I64 + _COL + _MAINT
            for k in names:
                self.ptrs[k] = self.records.ptr + int(off[order.index(k)])
        else:
            self.slot_bytes = 0
            for k in names:
                self.fields[k] = _abi.DeviceArray(self.ctx, self.shapes[k], self.dtypes[k])
                self.fields[k].zero()
                self.ptrs[k] = self.fields[k].ptr
        self._struct = _MapStruct(M, self.n_lobes, 0, *[self.ptrs.get(k) for k in _F64 + _I64 + _COL + _MAINT],
                                  self.slot_bytes)
        # per tile: every slot's rgb and colors = the fuse's estimate of its camera accumulators. Not so
        # for an empty tile (create_empty_tile: rgb gray, colors 0); a fuse leaves its tile current,
        # insert / merge / a colour upload do not
        self._tile_cc = [False] * self.n_tiles
        # pipelines with this map attached (BatchedScanPipeline.attach_primitive_map): told when a host
        # operation makes the colours stale, so their next in-scan update recomputes every slot's
        self._listeners: List[Any] = []
        if track_colors:
            self.upload(rgb=np.full((M, 3), 0.5))
        # AtlasMap bookkeeping (primitive_map.py:183-201): host integers, as in the reference
        self.next_global_id = 0
        self.total_count = 0
        self.tile_count: Dict[int, int] = {}
        # tile keys of the dense tiles (the reference's packed MA-hex tile ids); default 0..n-1
        self.tile_keys: List[int] = list(range(self.n_tiles))
        # tile residency (ensure_tiles): the tiles that are not resident, by key, and per slab the stamp
        # of the last ensure_tiles call that wanted its key
        self._store: Dict[int, _StoredTile] = {}
        self._last_used: List[int] = [0] * self.n_tiles
        self._use_clock = 0

    @property
    def colors_current(self) -> bool:
        """True while every slot's rgb / colors equal the fuse's estimate of its camera accumulators
        (a fuse then recomputes only the slots it touches, as gc_primitive_map.colors_current)."""
        return all(self._tile_cc)

    @colors_current.setter
    def colors_current(self, v: bool) -> None:
        if not v:
            self.colors_stale()
        else:
            self._tile_cc = [True] * self.n_tiles

    def colors_stale(self, tile_id: Optional[int] = None) -> None:
        """A host operation wrote colour fields (insert, merge, a colour upload): rgb / colors of the
        tile (None: every tile) are no longer the fuse's estimate. Attached pipelines are told, so
        their next in-scan update recomputes them (gc_pipeline_map_colors_stale)."""
        if tile_id is None:
            self._tile_cc = [False] * self.n_tiles
        else:
            self._tile_cc[int(tile_id)] = False
        alive = []
        for ref in self._listeners:
            pipe = ref()
            if pipe is not None and getattr(pipe, "_smap", None) is self:
                pipe._map_colors_stale()
                alive.append(ref)
        self._listeners = alive

    def struct(self) -> "_MapStruct":
        """The whole flat map (all tiles) for a C entry, its colour flag up to date."""
        self._struct.colors_current = 1 if self.colors_current else 0
        return self._struct

    def tile_struct(self, tile_id: int) -> "_MapStruct":
        """One tile as a map of m_tile slots (tile-local slot indices), as the reference's per-tile
        operators see it."""
        s0, n = self.tile_range(tile_id)
        st = _MapStruct.from_buffer_copy(self._struct)
        st.m_slots = n
        st.colors_current = 1 if self._tile_cc[int(tile_id)] else 0
        for k, p in self.ptrs.items():
            setattr(st, k, p + s0 * (self.slot_bytes or self._row_bytes(k)))
        return st

    def set_tile_keys(self, keys) -> None:
        keys = [int(k) for k in keys]
        if len(keys) != self.n_tiles or len(set(keys)) != len(keys):
            raise ValueError("tile keys must be n_tiles distinct ids")
        if any(k in self._store for k in keys):
            raise ValueError("a tile key of the host store cannot name a slab: ensure_tiles loads it")
        self.tile_keys = keys

    # ------------------------------------------------------------------------- tile residency
    def stored_keys(self) -> List[int]:
        """The keys of the tiles held by the host store (not resident)."""
        return list(self._store)

    def _attached(self) -> bool:
        for ref in self._listeners:
            pipe = ref()
            if pipe is not None and getattr(pipe, "_smap", None) is self:
                return True
        return False

    def ensure_tiles(self, keys) -> TileResidency:
        """Make every tile key of `keys` resident (plan_tile_residency): every victim is exported to the
        host store (always: upload() does not maintain tile_count, so the host cannot know a slab is
        empty), every incoming slab is imported from the store or reset to the empty tile, then
        tile_keys, tile_count, the colour flags and the store follow, and the stream is waited for once.
        When every key is resident nothing is launched and nothing is waited for. RuntimeError while a
        BatchedScanPipeline has the map attached: its in-scan update addresses flat slots."""
        keys = [int(k) for k in keys]
        if self._attached():
            raise RuntimeError("ensure_tiles while a pipeline has the map attached: detach it first "
                               "(attach_primitive_map(None))")
        plan = plan_tile_residency(self.tile_keys, self._last_used, keys, self._store.keys())
        hits = [k for k in keys if k in self.tile_keys]
        if plan:
            m, st = self.m_tile, self.struct()
            images = [np.empty(m * self.image_slot_bytes, np.uint8) for _ in plan]
            for mv, img in zip(plan, images):  # 1. every victim out
                _abi.call("gc_primitive_map_tile_export", self.ctx.handle, C.byref(st), mv.slab * m, m,
                          img.ctypes.data, ctx=self.ctx)
            for mv in plan:                    # 2. every incoming slab
                if mv.load:
                    _abi.call("gc_primitive_map_tile_import", self.ctx.handle, C.byref(st), mv.slab * m, m,
                              self._store[mv.incoming].image.ctypes.data, ctx=self.ctx)
                else:
                    _abi.call("gc_primitive_map_tile_reset", self.ctx.handle, C.byref(st), mv.slab * m, m,
                              ctx=self.ctx)
            loaded = []                        # 3. the bookkeeping; the loaded images live until the wait
            for mv, img in zip(plan, images):
                self._store[mv.evicted] = _StoredTile(img, self.tile_count.pop(mv.slab, None),
                                                      bool(self._tile_cc[mv.slab]))
            for mv in plan:
                self.tile_keys[mv.slab] = mv.incoming
                self._tile_cc[mv.slab] = False  # an empty tile: rgb gray, colors 0, as a new map
                if mv.load:
                    t = self._store.pop(mv.incoming)
                    loaded.append(t)
                    if t.tile_count is not None:
                        self.tile_count[mv.slab] = t.tile_count
                    self._tile_cc[mv.slab] = t.colors_current
            self.ctx.sync()                    # 4. the one wait
            del loaded
        self._use_clock += 1
        dense = [self.tile_keys.index(k) for k in keys]
        for d in dense:
            self._last_used[d] = self._use_clock
        return TileResidency(hits=hits, loaded=[mv.incoming for mv in plan if mv.load],
                             created=[mv.incoming for mv in plan if not mv.load],
                             evicted=[mv.evicted for mv in plan], dense=dense)

    def image_fields(self, image) -> Dict[str, np.ndarray]:
        """The fields this map holds out of a tile image (gc_primitive_map_tile_export), as download_tile
        returns them."""
        rec = np.asarray(image, np.uint8).reshape(-1, self.image_slot_bytes)
        order = _F64 + _I64 + _COL + _MAINT
        out = {}
        for k in self.ptrs:
            o, rb = int(self._image_off[order.index(k)]), self._row_bytes(k)
            out[k] = np.ascontiguousarray(rec[:, o:o + rb]).view(self.dtypes[k]).reshape(
                (rec.shape[0],) + self.shapes[k][1:])
        return out

    def key_fields(self, key: int) -> Dict[str, np.ndarray]:
        """The fields of the tile with key `key`, resident (a download) or in the host store."""
        d = self.dense_tile(key)
        if d >= 0:
            return self.download_tile(d)
        if int(key) not in self._store:
            raise KeyError(f"tile {key} is neither resident nor stored")
        return self.image_fields(self._store[int(key)].image)

    def key_count(self, key: int) -> Optional[int]:
        """tile_count of the tile with key `key`, resident or stored (None: never recorded)."""
        d = self.dense_tile(key)
        return self.tile_count.get(d) if d >= 0 else self._store[int(key)].tile_count

    def dense_tile(self, key: int) -> int:
        """Dense tile index holding tile key `key`, or -1 (an empty tile for the view)."""
        try:
            return self.tile_keys.index(int(key))
        except ValueError:
            return -1

    def _row_bytes(self, k: str) -> int:
        return int(np.prod(self.shapes[k][1:], dtype=np.int64)) * self.dtypes[k].itemsize

    def upload(self, **arrays):
        for k, v in arrays.items():
            if k not in self.ptrs:
                raise KeyError(k)
            if k in _COL:
                self.colors_stale()  # arbitrary colours / accumulators: the next fuse recomputes all
            if not self.packed:
                self.fields[k].upload(v)
                continue
            tmp = _abi.DeviceArray.from_host(self.ctx, np.asarray(v).reshape(self.shapes[k]), self.dtypes[k])
            rb = self._row_bytes(k)
            _abi.call("gc_copy_strided", self.ctx.handle, self.ptrs[k], self.slot_bytes, tmp.ptr, rb, rb, self.M,
                      ctx=self.ctx)
            self.ctx.sync()

    def download(self, *names):
        if not self.packed:
            return {k: self.fields[k].download() for k in (names or self.fields.keys())}
        out = {}
        for k in (names or self.ptrs.keys()):
            tmp = _abi.DeviceArray(self.ctx, self.shapes[k], self.dtypes[k])
            rb = self._row_bytes(k)
            _abi.call("gc_copy_strided", self.ctx.handle, tmp.ptr, rb, self.ptrs[k], self.slot_bytes, rb, self.M,
                      ctx=self.ctx)
            out[k] = tmp.download()
        return out

    def tile_slot(self, tile_id: int, slots) -> np.ndarray:
        return int(tile_id) * self.m_tile + np.asarray(slots, dtype=np.int64)

    def tile_range(self, tile_id: int) -> Tuple[int, int]:
        t = int(tile_id)
        if not 0 <= t < self.n_tiles:
            raise ValueError(f"tile_id {t} outside [0, {self.n_tiles})")
        return t * self.m_tile, self.m_tile

    def download_tile(self, tile_id: int, *names) -> Dict[str, np.ndarray]:
        s0, n = self.tile_range(tile_id)
        return {k: v[s0:s0 + n] for k, v in self.download(*names).items()}


@dataclass
class PrimitiveMapFuseResult:
    atlas_map: DevicePrimitiveMap
    tile_id: int
    n_fused: int


class DeviceFuseBatch:
    """K measurement rows resident in HBM (flat map slots), reusable across fuse calls."""

    def __init__(self, ctx, slots, Lambdas, thetas, etas, weights, responsibilities, valid_mask=None, colors=None,
                 sources=None, n_lobes: int = GC_VMF_N_LOBES):
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        K = self.K = sl.shape[0]
        arrs = [sl, np.ascontiguousarray(Lambdas, np.float64).reshape(K, 9),
                np.ascontiguousarray(thetas, np.float64).reshape(K, 3),
                np.ascontiguousarray(etas, np.float64).reshape(K, 3 * n_lobes),
                np.ascontiguousarray(weights, np.float64).reshape(K),
                np.ascontiguousarray(responsibilities, np.float64).reshape(K)]
        opt = [None if valid_mask is None else np.ascontiguousarray(valid_mask, np.uint8).reshape(K),
               None if colors is None else np.ascontiguousarray(colors, np.float64).reshape(K, 3),
               None if sources is None else np.ascontiguousarray(sources, np.int32).reshape(K)]
        self.dev = [_abi.DeviceArray.from_host(ctx, a, a.dtype) for a in arrs] + \
                   [_abi.DeviceArray.from_host(ctx, a, a.dtype) if a is not None else None for a in opt]
        self.struct = _FuseStruct(K, *[d.ptr if d is not None else None for d in self.dev])


def fuse_device(dmap: DevicePrimitiveMap, batch: DeviceFuseBatch, timestamp: float, scan_seq: int = 0,
                world_pose=None, eps_lift: float = GC_EPS_LIFT, eps_mass: float = GC_EPS_MASS,
                count: bool = True, tile_id: Optional[int] = None) -> int:
    """Fuse a resident batch in place; returns the distinct slots touched (count=False: -1, no sync).
    tile_id=None: the rows hold flat slots of the whole map; else tile-local slots of that tile (the
    colour estimate then covers that tile, as the reference's per-tile fuse)."""
    pose = None if world_pose is None else np.ascontiguousarray(world_pose, np.float64).reshape(6)
    n = C.c_int64(-1)
    st = dmap.struct() if tile_id is None else dmap.tile_struct(tile_id)
    _abi.call("gc_primitive_map_fuse", dmap.ctx.handle, C.byref(st), C.byref(batch.struct),
              None if pose is None else pose.ctypes.data, float(eps_lift), float(eps_mass), float(timestamp),
              int(scan_seq), C.byref(n) if count else None, ctx=dmap.ctx)
    if "cam_mass" in dmap.ptrs:  # the fuse leaves every slot's colour (of the tile) at its estimate
        if tile_id is None:
            dmap.colors_current = True
        else:
            dmap._tile_cc[int(tile_id)] = True
    return int(n.value)


def fuse_rows(dmap: DevicePrimitiveMap, slots, Lambdas, thetas, etas, weights, responsibilities, timestamp: float,
              scan_seq: int = 0, valid_mask=None, colors=None, sources=None, world_pose=None,
              eps_lift: float = GC_EPS_LIFT, eps_mass: float = GC_EPS_MASS, tile_id: Optional[int] = None) -> int:
    """K host rows (flat map slots, or tile-local with tile_id) -> fused in place; returns the number of
    distinct slots touched."""
    if np.asarray(slots).reshape(-1).shape[0] == 0:
        return 0
    b = DeviceFuseBatch(dmap.ctx, slots, Lambdas, thetas, etas, weights, responsibilities, valid_mask, colors,
                        sources, dmap.n_lobes)
    return fuse_device(dmap, b, timestamp, scan_seq, world_pose, eps_lift, eps_mass, tile_id=tile_id)


def primitive_map_fuse(atlas_map: DevicePrimitiveMap, tile_id: int, target_slots, Lambdas_meas, thetas_meas,
                       etas_meas, weights_meas, responsibilities, timestamp: float, scan_seq: int = 0,
                       valid_mask=None, colors_meas=None, sources_meas=None, eps_psd: float = GC_EPS_PSD,
                       eps_mass: float = GC_EPS_MASS, fuse_chunk_size: int = 0, chart_id: str = GC_CHART_ID,
                       anchor_id: str = "primitive_map", world_pose=None, eps_lift: float = GC_EPS_LIFT
                       ) -> Tuple[PrimitiveMapFuseResult, CertBundle, ExpectedEffect]:
    """Reference signature; fuse_chunk_size is accepted for compatibility (the device reduce-by-key
    has no chunking). world_pose (optional [t, rotvec]) applies transform_gaussian_to_world."""
    sl = np.asarray(target_slots, dtype=np.int64).reshape(-1)
    K = sl.shape[0]
    if K == 0:
        return (PrimitiveMapFuseResult(atlas_map, int(tile_id), 0),
                CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
                ExpectedEffect(objective_name="primitive_map_fuse", predicted=0.0, realized=0.0))
    atlas_map.tile_range(tile_id)  # validates the tile
    local = np.where((sl >= 0) & (sl < atlas_map.m_tile), sl, -1)
    n = fuse_rows(atlas_map, local, Lambdas_meas, thetas_meas, etas_meas, weights_meas, responsibilities, timestamp,
                  scan_seq, valid_mask, colors_meas if sources_meas is not None else None, sources_meas, world_pose,
                  eps_lift, eps_mass, tile_id=tile_id)
    return (PrimitiveMapFuseResult(atlas_map, int(tile_id), n),
            CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
            ExpectedEffect(objective_name="primitive_map_fuse", predicted=float(K), realized=float(n)))


# ----------------------------------------------------------------------------- maintenance
def _no_op(result, chart_id: str, anchor_id: str, name: str, predicted: float = 0.0):
    """_exact_no_op_result (primitive_map.py:624-640)."""
    return (result, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
            ExpectedEffect(objective_name=name, predicted=predicted, realized=0.0))


@dataclass
class PrimitiveMapForgetResult:
    atlas_map: DevicePrimitiveMap
    tile_id: int


def primitive_map_forget(atlas_map: DevicePrimitiveMap, tile_id: int,
                         forgetting_factor: float = GC_PRIMITIVE_FORGETTING_FACTOR, chart_id: str = GC_CHART_ID,
                         anchor_id: str = "primitive_map"
                         ) -> Tuple[PrimitiveMapForgetResult, CertBundle, ExpectedEffect]:
    """primitive_map_forget (primitive_map.py:1314-1390): weights *= γ on the tile."""
    s0, n = atlas_map.tile_range(tile_id)
    gamma = float(forgetting_factor)
    _abi.call("gc_primitive_map_forget", atlas_map.ctx.handle, C.byref(atlas_map.struct()), s0, n, gamma,
              ctx=atlas_map.ctx)
    return (PrimitiveMapForgetResult(atlas_map, int(tile_id)),
            CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
            ExpectedEffect(objective_name="primitive_map_forget", predicted=1.0 - gamma, realized=1.0 - gamma))


@dataclass
class PrimitiveMapRecencyInflateStats:
    staleness_inflation_strength: float
    staleness_cov_inflation_trace: float
    stale_precision_downscale_total: float
    per_tile: Optional[np.ndarray] = None  # (n, 3), the batched operator only: each visited tile's sums


def primitive_map_recency_inflate(atlas_map: DevicePrimitiveMap, tile_ids: List[int], scan_seq: int,
                                  recency_decay_lambda: float = GC_RECENCY_DECAY_LAMBDA,
                                  min_scale: float = GC_RECENCY_MIN_SCALE, chart_id: str = GC_CHART_ID,
                                  anchor_id: str = "primitive_map_recency_inflate"):
    """primitive_map_recency_inflate (primitive_map.py:1400-1490) -> (atlas_map, cert, effect, stats)."""
    n_valid = downscale = trace = 0.0
    for tid in tile_ids:
        s0, n = atlas_map.tile_range(tid)
        st = np.zeros(3)
        _abi.call("gc_primitive_map_recency_inflate", atlas_map.ctx.handle, C.byref(atlas_map.struct()), s0, n,
                  int(scan_seq), float(recency_decay_lambda), float(min_scale), st.ctypes.data, ctx=atlas_map.ctx)
        n_valid += st[0]
        downscale += st[1]
        trace += st[2]
    stats = PrimitiveMapRecencyInflateStats(staleness_inflation_strength=float(downscale / max(n_valid, 1.0)),
                                            staleness_cov_inflation_trace=float(trace),
                                            stale_precision_downscale_total=float(downscale))
    return (atlas_map, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
            ExpectedEffect(objective_name="primitive_map_recency_inflate", predicted=float(n_valid),
                           realized=float(n_valid)), stats)


def _recency_tiles_dense(atlas_map: DevicePrimitiveMap, tile_keys) -> List[int]:
    """The dense tiles of the keys the batched inflate visits: a key the map does not know is skipped
    (primitive_map.py:1420-1424), a key of the host store is an error."""
    dense = []
    for k in tile_keys:
        d = atlas_map.dense_tile(int(k))
        if d < 0:
            if int(k) in atlas_map._store:
                raise ValueError(f"tile {int(k)} is in the host store, not resident: ensure_tiles first")
            continue
        dense.append(d)
    if len(set(dense)) != len(dense):
        raise ValueError(f"duplicate tile keys in {[int(k) for k in tile_keys]}")
    if dense and "valid_mask" not in atlas_map.ptrs:
        raise ValueError("the map has no maintenance fields")
    return dense


def _recency_tiles_launch(atlas_map: DevicePrimitiveMap, d_dense, h_dense: np.ndarray, scan_seq: int,
                          recency_decay_lambda: float, min_scale: float, d_stats) -> None:
    """gc_primitive_map_recency_inflate_tiles on the map's stream: no download, no wait."""
    _abi.call("gc_primitive_map_recency_inflate_tiles", atlas_map.ctx.handle, C.byref(atlas_map.struct()),
              atlas_map.m_tile, int(h_dense.shape[0]), d_dense.ptr, h_dense.ctypes.data, int(scan_seq),
              float(recency_decay_lambda), float(min_scale), d_stats.ptr, ctx=atlas_map.ctx)


def _recency_tiles_finish(atlas_map, per_tile: np.ndarray, chart_id: str, anchor_id: str):
    """The operator's return from the per-tile statistics (n, 3), added in tile order as the reference's
    loop adds them (primitive_map.py:1425-1470)."""
    st = np.asarray(per_tile, np.float64).reshape(-1, 3)
    n_valid = downscale = trace = 0.0
    for row in st:
        n_valid += row[0]
        downscale += row[1]
        trace += row[2]
    stats = PrimitiveMapRecencyInflateStats(staleness_inflation_strength=float(downscale / max(n_valid, 1.0)),
                                            staleness_cov_inflation_trace=float(trace),
                                            stale_precision_downscale_total=float(downscale), per_tile=st.copy())
    return (atlas_map, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
            ExpectedEffect(objective_name="primitive_map_recency_inflate", predicted=float(n_valid),
                           realized=float(n_valid)), stats)


def primitive_map_recency_inflate_tiles(atlas_map: DevicePrimitiveMap, tile_keys, scan_seq: int,
                                        recency_decay_lambda: float = GC_RECENCY_DECAY_LAMBDA,
                                        min_scale: float = GC_RECENCY_MIN_SCALE, chart_id: str = GC_CHART_ID,
                                        anchor_id: str = "primitive_map_recency_inflate"):
    """primitive_map_recency_inflate (primitive_map.py:1400-1490) over the tiles with keys `tile_keys` in
    one device pass (gc_primitive_map_recency_inflate_tiles) and one download -> (atlas_map, cert,
    effect, stats), with the map and the bits of the per-tile operator looped over the same tiles;
    stats.per_tile holds [n_valid, Σ(1 - decay), Σ(1/decay - 1)] of each visited tile. A key the map does
    not know is skipped, as the reference skips a missing tile; a key that is in the host store but not
    resident raises ValueError."""
    dense = _recency_tiles_dense(atlas_map, tile_keys)
    if not dense:
        return _recency_tiles_finish(atlas_map, np.zeros((0, 3)), chart_id, anchor_id)
    h_dense = np.asarray(dense, np.int32)
    d_dense, = _abi.upload_many(atlas_map.ctx, [h_dense], [np.int32])
    d_stats = _abi.DeviceArray(atlas_map.ctx, (len(dense), 3), np.float64)
    _recency_tiles_launch(atlas_map, d_dense, h_dense, scan_seq, recency_decay_lambda, min_scale, d_stats)
    return _recency_tiles_finish(atlas_map, d_stats.download(), chart_id, anchor_id)  # the one download


@dataclass
class PrimitiveMapCullResult:
    atlas_map: DevicePrimitiveMap
    tile_id: int
    n_culled: int
    mass_dropped: float


def primitive_map_cull(atlas_map: DevicePrimitiveMap, tile_id: int,
                       weight_threshold: float = GC_PRIMITIVE_CULL_WEIGHT_THRESHOLD,
                       max_primitives: Optional[int] = None, chart_id: str = GC_CHART_ID,
                       anchor_id: str = "primitive_map") -> Tuple[PrimitiveMapCullResult, CertBundle, ExpectedEffect]:
    """primitive_map_cull (primitive_map.py:1175-1305)."""
    s0, n = atlas_map.tile_range(tile_id)
    out = np.zeros(4)
    _abi.call("gc_primitive_map_cull", atlas_map.ctx.handle, C.byref(atlas_map.struct()), s0, n,
              float(weight_threshold), -1 if max_primitives is None else int(max_primitives), out.ctypes.data,
              ctx=atlas_map.ctx)
    return _cull_finish(atlas_map, int(tile_id), int(out[3]), int(out[0]), float(out[1]), float(out[2]), chart_id,
                        anchor_id)


def _cull_finish(atlas_map, tile_id: int, n_valid: int, n_culled: int, mass_dropped: float, sum_w: float,
                 chart_id: str, anchor_id: str):
    """The bookkeeping, certificate and effect of a cull from its device counts (primitive_map.py:1240-1305)."""
    if n_valid == 0 or n_culled == 0:
        return _no_op(PrimitiveMapCullResult(atlas_map, tile_id, 0, 0.0), chart_id, anchor_id, "primitive_map_cull")
    atlas_map.tile_count[tile_id] = n_valid - n_culled
    atlas_map.total_count -= n_culled
    cert = CertBundle.create_approx(chart_id=chart_id, anchor_id=anchor_id, triggers=["budgeting", "mass_drop"],
                                    influence=InfluenceCert.identity().with_overrides(
                                        mass_epsilon_ratio=mass_dropped / (sum_w + GC_EPS_MASS)))
    return (PrimitiveMapCullResult(atlas_map, tile_id, n_culled, mass_dropped), cert,
            ExpectedEffect(objective_name="primitive_map_cull", predicted=float(n_culled), realized=float(n_culled)))


@dataclass
class PrimitiveMapInsertResult:
    atlas_map: DevicePrimitiveMap
    tile_id: int
    n_inserted: int
    new_ids: np.ndarray
    target_slots: Optional[np.ndarray] = None  # tile-local eviction slots (extra field)


def primitive_map_insert_masked(atlas_map: DevicePrimitiveMap, tile_id: int, Lambdas_new, thetas_new, etas_new,
                                weights_new, timestamp: float, valid_new_mask, scan_seq: int = 0,
                                recency_decay_lambda: float = GC_RECENCY_DECAY_LAMBDA, colors_new=None,
                                sources_new=None, chart_id: str = GC_CHART_ID,
                                anchor_id: str = "primitive_map_insert_masked"
                                ) -> Tuple[PrimitiveMapInsertResult, CertBundle, ExpectedEffect]:
    """primitive_map_insert_masked (primitive_map.py:807-982)."""
    s0, n = atlas_map.tile_range(tile_id)
    L = atlas_map.n_lobes
    w = np.ascontiguousarray(weights_new, np.float64).reshape(-1)
    K = w.shape[0]
    mask = np.ascontiguousarray(valid_new_mask).reshape(-1).astype(np.uint8)
    if mask.shape[0] != K or K > n or K == 0:
        raise ValueError(f"insert_masked: K={K} proposals, mask {mask.shape[0]}, tile {n}")
    ctx = atlas_map.ctx
    arrs = [np.ascontiguousarray(Lambdas_new, np.float64).reshape(K, 9),
            np.ascontiguousarray(thetas_new, np.float64).reshape(K, 3),
            np.ascontiguousarray(etas_new, np.float64).reshape(K, 3 * L), w, mask,
            None if colors_new is None else np.ascontiguousarray(colors_new, np.float64).reshape(K, 3),
            None if sources_new is None else np.ascontiguousarray(sources_new, np.int32).reshape(K)]
    dev = [None if a is None else _abi.DeviceArray.from_host(ctx, a, a.dtype) for a in arrs]
    batch = _InsertStruct(K, *[None if d is None else d.ptr for d in dev])
    d_slots = _abi.DeviceArray(ctx, K, np.int32)
    d_ids = _abi.DeviceArray(ctx, K, np.int64)
    out = np.zeros(2, np.int64)
    _abi.call("gc_primitive_map_insert_masked", ctx.handle, C.byref(atlas_map.struct()), s0, n, C.byref(batch),
              float(timestamp), int(scan_seq), float(recency_decay_lambda), int(atlas_map.next_global_id),
              d_slots.ptr, d_ids.ptr, out.ctypes.data, ctx=ctx)
    n_ins, count = int(out[0]), int(out[1])
    if n_ins > 0:
        atlas_map.colors_stale(tile_id)  # inserted colours are clip(c), not the estimate clip(c·cam / cam)
    atlas_map.next_global_id += n_ins
    atlas_map.total_count += n_ins
    atlas_map.tile_count[int(tile_id)] = count
    dropped = int(np.sum(mask == 0))
    cert = (CertBundle.create_approx(chart_id=chart_id, anchor_id=anchor_id, triggers=["insert_unfilled_budget"],
                                     frobenius_applied=False) if dropped > 0
            else CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id))
    return (PrimitiveMapInsertResult(atlas_map, int(tile_id), n_ins, d_ids.download(), d_slots.download()), cert,
            ExpectedEffect(objective_name="primitive_map_insert_masked", predicted=float(int(mask.sum())),
                           realized=float(n_ins)))


@dataclass
class PrimitiveMapMergeReduceResult:
    atlas_map: DevicePrimitiveMap
    tile_id: int
    n_merged: int
    frobenius_correction: float


def primitive_map_merge_reduce(atlas_map: DevicePrimitiveMap, tile_id: int,
                               merge_threshold: float = GC_PRIMITIVE_MERGE_THRESHOLD,
                               max_pairs: int = GC_K_MERGE_PAIRS_PER_TILE,
                               max_tile_size: int = GC_PRIMITIVE_MERGE_MAX_TILE_SIZE, eps_psd: float = GC_EPS_PSD,
                               eps_lift: float = GC_EPS_LIFT, chart_id: str = GC_CHART_ID,
                               anchor_id: str = "primitive_map"
                               ) -> Tuple[PrimitiveMapMergeReduceResult, CertBundle, ExpectedEffect]:
    """primitive_map_merge_reduce (primitive_map.py:1809-2030)."""
    s0, M = atlas_map.tile_range(tile_id)
    if int(max_tile_size) > 0 and M > int(max_tile_size):
        # the budget cap (:1881-1890) applies after the M / valid count / max_pairs no-op test (:1879)
        n_valid = int(atlas_map.download_tile(tile_id, "valid_mask")["valid_mask"].sum())
        state = _MM_NOOP if M < 2 or n_valid < 2 or int(max_pairs) <= 0 else _MM_CAPPED
        return _merge_finish(atlas_map, int(tile_id), state, 0, 0, int(max_pairs), int(max_tile_size), chart_id,
                             anchor_id)
    out = np.zeros(2, np.int64)
    _abi.call("gc_primitive_map_merge_reduce", atlas_map.ctx.handle, C.byref(atlas_map.struct()), s0, M,
              float(merge_threshold), int(max_pairs), float(eps_psd), float(eps_lift), out.ctypes.data,
              ctx=atlas_map.ctx)
    return _merge_finish(atlas_map, int(tile_id), _MM_RAN, int(out[0]), int(out[1]), int(max_pairs),
                         int(max_tile_size), chart_id, anchor_id)


_MM_RAN, _MM_NOOP, _MM_CAPPED = 0, 1, 2  # GC_MAP_MAINTAIN_MERGE_*


def _merge_finish(atlas_map, tile_id: int, state: int, n_merged: int, count: int, max_pairs: int,
                  max_tile_size: int, chart_id: str, anchor_id: str):
    """The bookkeeping, certificate and effect of a merge-reduce from its outcome (primitive_map.py:1879-1890,
    :1985-2030): the exact no-op, the budget cap, or n_merged pairs leaving `count` valid slots."""
    M = atlas_map.m_tile

    def no_op(predicted, triggers=None, influence=None):
        res = PrimitiveMapMergeReduceResult(atlas_map, tile_id, 0, 0.0)
        cert = (CertBundle.create_approx(chart_id=chart_id, anchor_id=anchor_id, triggers=triggers,
                                         frobenius_applied=True, influence=influence or InfluenceCert.identity())
                if triggers else CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id))
        return res, cert, ExpectedEffect(objective_name="primitive_map_merge_reduce", predicted=predicted,
                                         realized=0.0)

    if state == _MM_CAPPED:
        over = float(M - max_tile_size) / float(max(M, 1))
        return no_op(float(max_pairs), ["merge_reduce_budget_cap"],
                     InfluenceCert.identity().with_overrides(mass_epsilon_ratio=over))
    if state == _MM_NOOP or n_merged <= 0:
        return no_op(float(max_pairs))
    atlas_map.colors_stale(tile_id)  # merged colours use max(denom, eps_psd) (primitive_map.py:1976-1983)
    atlas_map.tile_count[tile_id] = count
    atlas_map.total_count -= n_merged
    cert = CertBundle.create_approx(chart_id=chart_id, anchor_id=anchor_id, triggers=["primitive_map_merge_reduce"],
                                    frobenius_applied=True, influence=InfluenceCert.identity().with_overrides(
                                        mass_epsilon_ratio=float(n_merged) / float(max(M, 1))))
    return (PrimitiveMapMergeReduceResult(atlas_map, tile_id, n_merged, float(n_merged)), cert,
            ExpectedEffect(objective_name="primitive_map_merge_reduce", predicted=float(max_pairs),
                           realized=float(n_merged)))


# ----------------------------------------------------------------------------- the post-pose map update
_MU_HEAD, _MU_TILE = GC_MAP_UPDATE_STATS_HEAD, GC_MAP_UPDATE_STATS_TILE

_MU_BATCH = (("Lambdas", np.float64, 9), ("thetas", np.float64, 3), ("etas", np.float64, None),
             ("weights", np.float64, 1), ("valid_mask", np.uint8, 1), ("colors", np.float64, 3),
             ("sources", np.int32, 1))
_MU_ASSOC = (("responsibilities", np.float64), ("candidate_tile_ids", np.int64), ("candidate_slots", np.int64),
             ("row_masses", np.float64))


_MapUpdateIn = _abi.STRUCTS["gc_map_update_in"]  # its pointers: _MU_BATCH, _MU_ASSOC, then the active tiles
_MapUpdateOut = _abi.STRUCTS["gc_map_update_out"]


@dataclass
class MapUpdateConfig:
    """The PipelineConfig fields step 12b reads (pipeline.py:96-160)."""
    k_insert_tile: int = GC_K_INSERT_TILE
    h_tile: float = GC_H_TILE
    block_size: int = GC_ASSOC_BLOCK_SIZE
    eps_lift: float = GC_EPS_LIFT
    eps_mass: float = GC_EPS_MASS
    eps_psd: float = GC_EPS_PSD
    recency_decay_lambda: float = GC_RECENCY_DECAY_LAMBDA
    primitive_cull_weight_threshold: float = GC_PRIMITIVE_CULL_WEIGHT_THRESHOLD
    primitive_forgetting_factor: float = GC_PRIMITIVE_FORGETTING_FACTOR
    primitive_merge_threshold: float = GC_PRIMITIVE_MERGE_THRESHOLD
    k_merge_pairs_tile: int = GC_K_MERGE_PAIRS_PER_TILE
    max_tile_size: int = GC_PRIMITIVE_MERGE_MAX_TILE_SIZE


_MM_TILE = GC_MAP_MAINTAIN_STATS_TILE


@dataclass
class PrimitiveMapMaintainResult:
    """Cull / forget / merge-reduce of the active tiles, one entry per tile in the given order."""
    atlas_map: DevicePrimitiveMap
    tile_ids: List[int]
    n_culled: np.ndarray      # (n_active,) int64
    mass_dropped: np.ndarray  # (n_active,) float64
    n_merged: np.ndarray      # (n_active,) int64
    n_culled_total: int
    mass_dropped_total: float
    n_merged_total: int
    tile_certs: List[Tuple[CertBundle, CertBundle, CertBundle]]  # per tile: (cull, forget, merge)


def _maintain_check(atlas_map, dense: List[int], cfg: MapUpdateConfig) -> None:
    """The argument errors of the batched maintenance, raised before any device call."""
    if len(set(dense)) != len(dense):
        raise ValueError(f"duplicate tile ids in {dense}")
    n_tiles = len(atlas_map.tile_keys)
    for d in dense:
        if not 0 <= d < n_tiles:
            raise ValueError(f"tile_id {d} outside [0, {n_tiles})")
    if "valid_mask" not in atlas_map.ptrs:
        raise ValueError("the map has no maintenance fields")
    M, cap = atlas_map.m_tile, int(cfg.max_tile_size)
    runs = M >= 2 and int(cfg.k_merge_pairs_tile) > 0 and not (cap > 0 and M > cap)
    if runs and M > 65536:
        raise ValueError(f"merge-reduce of tiles of {M} slots: at most 65536")


def _maintain_launch(atlas_map, d_dense, h_dense: np.ndarray, cfg: MapUpdateConfig, max_primitives: Optional[int],
                     max_sort_keys: int, d_stats) -> None:
    """gc_primitive_map_maintain on the map's stream: no download, no wait."""
    _abi.call("gc_primitive_map_maintain", atlas_map.ctx.handle, C.byref(atlas_map.struct()), atlas_map.m_tile,
              int(h_dense.shape[0]), d_dense.ptr, h_dense.ctypes.data, C.byref(_abi.cfg("gc_map_maintain_cfg", cfg)),
              -1 if max_primitives is None else int(max_primitives), int(cfg.k_merge_pairs_tile),
              int(cfg.max_tile_size), int(max_sort_keys), d_stats.ptr, ctx=atlas_map.ctx)


def _maintain_finish(atlas_map, dense: List[int], stats: np.ndarray, cfg: MapUpdateConfig, chart_id: str
                     ) -> PrimitiveMapMaintainResult:
    """The bookkeeping and the certificates the loop of per-tile operators would have left, from the
    statistics of the one pass (tiles in order; cull, forget, merge of each)."""
    st = np.asarray(stats, np.float64).reshape(len(dense), _MM_TILE)
    n_culled, mass, n_merged, certs = [], [], [], []
    for a, d in enumerate(dense):
        rc, cc, _ = _cull_finish(atlas_map, d, int(st[a, 0]), int(st[a, 1]), float(st[a, 2]), float(st[a, 3]),
                                 chart_id, "primitive_map")
        cf = CertBundle.create_exact(chart_id=chart_id, anchor_id="primitive_map")
        rm, cm, _ = _merge_finish(atlas_map, d, int(st[a, 7]), int(st[a, 5]), int(st[a, 6]),
                                  int(cfg.k_merge_pairs_tile), int(cfg.max_tile_size), chart_id,
                                  "primitive_map_merge_reduce")
        n_culled.append(int(rc.n_culled))
        mass.append(float(rc.mass_dropped))
        n_merged.append(int(rm.n_merged))
        certs.append((cc, cf, cm))
    evicted = 0.0
    for m in mass:  # summed in tile order, as the loop does
        evicted += m
    return PrimitiveMapMaintainResult(
        atlas_map=atlas_map, tile_ids=list(dense), n_culled=np.asarray(n_culled, np.int64),
        mass_dropped=np.asarray(mass, np.float64), n_merged=np.asarray(n_merged, np.int64),
        n_culled_total=int(sum(n_culled)), mass_dropped_total=evicted, n_merged_total=int(sum(n_merged)),
        tile_certs=certs)


def primitive_map_maintain(atlas_map: DevicePrimitiveMap, tile_ids, config: Optional[MapUpdateConfig] = None,
                           max_primitives: Optional[int] = None, max_sort_keys: int = 0,
                           chart_id: str = GC_CHART_ID
                           ) -> Tuple[PrimitiveMapMaintainResult, CertBundle, ExpectedEffect]:
    """The maintenance of step 12b (pipeline.py:1412-1447) over the dense tiles `tile_ids` in one device
    pass (gc_primitive_map_maintain) and one download: per tile primitive_map_cull, primitive_map_forget
    and primitive_map_merge_reduce (anchor "primitive_map_merge_reduce"), with the map, the bookkeeping
    and the certificates the loop of those operators leaves. max_sort_keys bounds the merge's scratch
    (pair keys sorted at once; 0 = the library's default)."""
    from .certificates import aggregate_certificates
    cfg = config or MapUpdateConfig()
    dense = [int(t) for t in tile_ids]
    _maintain_check(atlas_map, dense, cfg)
    predicted = float(len(dense) * int(cfg.k_merge_pairs_tile))
    if not dense:
        z = np.zeros(0)
        return (PrimitiveMapMaintainResult(atlas_map, [], z.astype(np.int64), z, z.astype(np.int64), 0, 0.0, 0, []),
                CertBundle.create_exact(chart_id=chart_id, anchor_id="primitive_map"),
                ExpectedEffect(objective_name="primitive_map_maintain", predicted=0.0, realized=0.0))
    ctx = atlas_map.ctx
    h_dense = np.asarray(dense, np.int32)
    d_dense, = _abi.upload_many(ctx, [h_dense], [np.int32])
    d_stats = _abi.DeviceArray(ctx, (len(dense) * _MM_TILE,), np.float64)
    _maintain_launch(atlas_map, d_dense, h_dense, cfg, max_primitives, max_sort_keys, d_stats)
    res = _maintain_finish(atlas_map, dense, d_stats.download(), cfg, chart_id)  # the one download
    cert = aggregate_certificates([c for t in res.tile_certs for c in t])
    return res, cert, ExpectedEffect(objective_name="primitive_map_maintain", predicted=predicted,
                                     realized=float(res.n_merged_total))


@dataclass
class PrimitiveMapUpdateResult:
    """The counters of pipeline.py:930-937 and the insert plan, one row per active tile."""
    atlas_map: DevicePrimitiveMap
    n_fused: int
    n_inserted: int
    n_culled: int
    n_merged: int
    fused_mass_total: float
    insert_mass_total: float
    insert_mass_p95: float
    evicted_mass_total: float
    insert_indices: np.ndarray       # (n_active, k_insert_tile) int32 measurement rows
    insert_valid: np.ndarray         # (n_active, k_insert_tile) bool, valid_new after the placeholder rule
    insert_target_slots: np.ndarray  # (n_active, k_insert_tile) int32 tile-local eviction slots
    new_ids: np.ndarray              # (n_active, k_insert_tile) int64, -1 where not inserted
    event_log_entries: Optional[List[dict]] = None


def _mu_shape(x):
    return tuple(x.shape) if isinstance(x, _abi.DeviceArray) else np.shape(x)


def primitive_map_update_from_association(atlas_map: DevicePrimitiveMap, association_result, measurement_batch,
                                          active_tile_ids, pose_world, timestamp: float, scan_seq: int,
                                          config: Optional[MapUpdateConfig] = None,
                                          map_branch_stats: Optional[dict] = None, maintenance=True,
                                          event_log: bool = False, chart_id: str = GC_CHART_ID
                                          ) -> Tuple[PrimitiveMapUpdateResult, CertBundle, ExpectedEffect]:
    """Step 12b of the reference (backend/pipeline.py:1232-1492) with z_t = pose_world = [t, rotvec]:
    the per-block, per-tile fuse of the associated rows (:1258-1327), the per-tile novelty insert
    (:1331-1410), then cull / forget / merge-reduce of every active tile (:1412-1447) and the
    MapUpdateCert (:1454-1487). active_tile_ids are tile keys of atlas_map in
    ma_hex_stencil_tile_ids order. The fuse and the inserts run in one device pass
    (gc_primitive_map_update) with one download at its end; the association's and the batch's
    `.device` arrays are read in place, host arrays are uploaded. map_branch_stats: the six floats
    the map branch hands to the certificate (pipeline.py:920-925). maintenance: False skips cull /
    forget / merge-reduce, True runs them through the per-tile operators (each waits for its counts),
    "device" chains gc_primitive_map_maintain behind the update on the same stream, its statistics
    in the same download: all of step 12b in one pass and one wait, with the same results."""
    cfg = config or MapUpdateConfig()
    ctx = atlas_map.ctx
    keys = [int(t) for t in active_tile_ids]
    if len(set(keys)) != len(keys):
        raise ValueError(f"duplicate active tile ids in {keys}")
    dense = [atlas_map.dense_tile(t) for t in keys]
    if any(d < 0 for d in dense):
        raise ValueError(f"active tile {keys[[d < 0 for d in dense].index(True)]} is not a tile of the map")
    n_active, k_ins, m_tile = len(keys), int(cfg.k_insert_tile), atlas_map.m_tile
    adev = getattr(association_result, "device", None)
    assoc = {k: (adev[k] if adev is not None else getattr(association_result, k)) for k, _ in _MU_ASSOC}
    if len(_mu_shape(assoc["responsibilities"])) != 2:
        raise ValueError(f"responsibilities must be (N, K), got {_mu_shape(assoc['responsibilities'])}")
    N, K = (int(v) for v in _mu_shape(assoc["responsibilities"]))
    for k in ("candidate_tile_ids", "candidate_slots"):
        if _mu_shape(assoc[k]) != (N, K):
            raise ValueError(f"{k} of shape {_mu_shape(assoc[k])}, expected {(N, K)}")
    if int(np.prod(_mu_shape(assoc["row_masses"]))) != N:
        raise ValueError(f"row_masses of shape {_mu_shape(assoc['row_masses'])}, expected {(N,)}")
    mdev = getattr(measurement_batch, "device", None)
    batch = {}
    for k, _, _ in _MU_BATCH:
        v = mdev.get(k) if mdev is not None else getattr(measurement_batch, k, None)
        if v is None:
            if k not in ("colors", "sources"):
                raise ValueError(f"the measurement batch has no {k}")
            v = np.zeros((N, 3)) if k == "colors" else np.ones(N, np.int32)  # no colour column: all LiDAR
        batch[k] = v
    eshape = _mu_shape(batch["etas"])
    if len(eshape) != 3 or eshape[1] != atlas_map.n_lobes or eshape[2] != 3:
        raise ValueError(f"etas of shape {eshape}: the map holds {atlas_map.n_lobes} lobes")
    for k, _, w in _MU_BATCH:
        n = _mu_shape(batch[k])[0] if len(_mu_shape(batch[k])) else -1
        if n != N:
            raise ValueError(f"measurement batch {k} has {n} rows, the association {N}")
    if not 1 <= k_ins <= min(N, m_tile):
        raise ValueError(f"k_insert_tile = {k_ins} outside [1, min(N = {N}, m_tile = {m_tile})]")
    if N > GC_MAP_UPDATE_MAX_ROWS or k_ins > GC_MAP_UPDATE_MAX_INSERT or n_active > GC_MAP_UPDATE_MAX_ACTIVE or \
            not 1 <= K <= GC_MAP_UPDATE_MAX_K:
        raise ValueError(f"beyond the insert plan's bounds: N = {N} <= {GC_MAP_UPDATE_MAX_ROWS}, k_insert_tile = "
                         f"{k_ins} <= {GC_MAP_UPDATE_MAX_INSERT}, {n_active} active tiles <= "
                         f"{GC_MAP_UPDATE_MAX_ACTIVE}, K = {K} in [1, {GC_MAP_UPDATE_MAX_K}]")
    pose = np.ascontiguousarray(pose_world, np.float64).reshape(-1)
    if pose.shape[0] != 6 or not np.all(np.isfinite(pose)):
        raise ValueError(f"pose_world must be 6 finite values [t, rotvec], got {pose}")
    if not float(cfg.h_tile) > 0.0:
        raise ValueError(f"h_tile must be > 0, got {cfg.h_tile}")
    if int(cfg.block_size) < 1:
        raise ValueError(f"block_size must be >= 1, got {cfg.block_size}")
    if "valid_mask" not in atlas_map.ptrs:
        raise ValueError("the map has no maintenance fields")
    on_device = isinstance(maintenance, str)
    if on_device:
        if maintenance != "device":
            raise ValueError(f"maintenance must be True, False or 'device', got {maintenance!r}")
        _maintain_check(atlas_map, dense, cfg)
    mb = dict(map_branch_stats or {})
    L = atlas_map.n_lobes
    AK = n_active * k_ins
    n_stats = _MU_HEAD + _MU_TILE * n_active
    if n_active:
        h_dense = np.asarray(dense, np.int32)
        host_in = [batch[k] if isinstance(batch[k], _abi.DeviceArray) else
                   np.ascontiguousarray(batch[k], dt).reshape((N,) if w == 1 else (N, w or 3 * L))
                   for k, dt, w in _MU_BATCH] + \
                  [assoc[k] if isinstance(assoc[k], _abi.DeviceArray) else
                   np.ascontiguousarray(assoc[k], dt).reshape((N,) if k == "row_masses" else (N, K))
                   for k, dt in _MU_ASSOC] + [np.asarray(keys, np.int64), h_dense]
        dts = [dt for _, dt, _ in _MU_BATCH] + [dt for _, dt in _MU_ASSOC] + [np.int64, np.int32]
        d_in = _abi.upload_many(ctx, host_in, dts)
        d_out = _abi.alloc_many(ctx, [((AK,), np.int32), ((AK,), np.uint8), ((AK,), np.int32), ((AK,), np.int64),
                                      ((AK, 9), np.float64), ((AK, 3), np.float64), ((AK,), np.float64),
                                      ((n_stats,), np.float64)] +
                                ([((n_active * _MM_TILE,), np.float64)] if on_device else []))
        s_in = _MapUpdateIn(N, m_tile, K, n_active, k_ins, int(cfg.block_size), *[d.ptr for d in d_in],
                            h_dense.ctypes.data)
        s_out = _MapUpdateOut(*[d.ptr for d in d_out[:8]])
        _abi.call("gc_primitive_map_update", ctx.handle, C.byref(atlas_map.struct()), C.byref(s_in), pose.ctypes.data,
                  C.byref(_abi.cfg("gc_map_update_cfg", cfg)), float(timestamp), int(scan_seq),
                  int(atlas_map.next_global_id), C.byref(s_out), ctx=ctx)
        if on_device:  # behind the last insert, on the same stream
            _maintain_launch(atlas_map, d_in[-1], h_dense, cfg, None, 0, d_out[8])
        idx, val, slots, ids, pL, pth, pw, stats, *mstats = _abi.download_many(d_out)  # the one download
    else:
        idx, val, slots, ids = (np.zeros(0, t) for t in (np.int32, np.uint8, np.int32, np.int64))
        pL, pth, pw, stats, mstats = np.zeros((0, 9)), np.zeros((0, 3)), np.zeros(0), np.zeros(n_stats), [np.zeros(0)]
    tiles = stats[_MU_HEAD:].reshape(n_active, _MU_TILE)
    n_fused = n_active * int(stats[1])
    n_inserted, mass_total, mass_p95 = 0, 0.0, 0.0
    for a, d in enumerate(dense):
        n_ins = int(tiles[a, 1])
        atlas_map.tile_count[d] = int(tiles[a, 0])
        atlas_map.total_count += n_ins
        atlas_map.next_global_id += n_ins
        n_inserted += n_ins
        mass_total += float(tiles[a, 2])            # pipeline.py:1366
        mass_p95 = max(mass_p95, float(tiles[a, 3]))  # :1367-1371
        if "cam_mass" in atlas_map.ptrs:
            atlas_map._tile_cc[d] = True            # the fuse left every slot of the tile at its estimate
            if n_ins > 0:
                atlas_map.colors_stale(d)           # inserted colours are clip(c), as primitive_map_insert_masked
    entries: Optional[List[dict]] = None
    if event_log:  # pipeline.py:1393-1410: every proposal of a tile that inserted any
        entries = []
        col = _abi.host(batch["colors"]).reshape(N, 3)
        for a in range(n_active):
            if int(tiles[a, 1]) <= 0:
                continue
            sl = slice(a * k_ins, (a + 1) * k_ins)
            mu = np.linalg.solve(pL[sl].reshape(-1, 3, 3) + cfg.eps_lift * np.eye(3)[None], pth[sl][..., None])[..., 0]
            for q in range(k_ins):
                entries.append({"tile_id": keys[a], "mu_world": mu[q].tolist(), "weight": float(pw[sl][q]),
                                "color": col[idx[sl][q]].tolist(), "timestamp": float(timestamp)})
    n_culled, n_merged, evicted = 0, 0, 0.0
    if on_device:  # pipeline.py:1412-1447 from the pass's statistics
        mr = _maintain_finish(atlas_map, dense, mstats[0], cfg, chart_id)
        n_culled, n_merged, evicted = mr.n_culled_total, mr.n_merged_total, mr.mass_dropped_total
    elif maintenance:  # pipeline.py:1412-1447, per active tile in order
        for d in dense:
            rc, _, _ = primitive_map_cull(atlas_map, d, cfg.primitive_cull_weight_threshold, chart_id=chart_id)
            n_culled += int(rc.n_culled)
            evicted += float(rc.mass_dropped)
            primitive_map_forget(atlas_map, d, cfg.primitive_forgetting_factor, chart_id=chart_id)
            rm, _, _ = primitive_map_merge_reduce(atlas_map, d, cfg.primitive_merge_threshold,
                                                  int(cfg.k_merge_pairs_tile), int(cfg.max_tile_size), cfg.eps_psd,
                                                  cfg.eps_lift, chart_id=chart_id,
                                                  anchor_id="primitive_map_merge_reduce")
            n_merged += int(rm.n_merged)
    result = PrimitiveMapUpdateResult(
        atlas_map=atlas_map, n_fused=n_fused, n_inserted=n_inserted, n_culled=n_culled, n_merged=n_merged,
        fused_mass_total=float(stats[0]), insert_mass_total=mass_total, insert_mass_p95=mass_p95,
        evicted_mass_total=evicted, insert_indices=idx.reshape(n_active, k_ins).copy(),
        insert_valid=val.reshape(n_active, k_ins).astype(bool),
        insert_target_slots=slots.reshape(n_active, k_ins).copy(), new_ids=ids.reshape(n_active, k_ins).copy(),
        event_log_entries=entries)
    active = set(keys)
    inactive = [int(t) for t in atlas_map.tile_keys if int(t) not in active]
    hits = len([t for t in keys if t in atlas_map.tile_keys])
    cert = CertBundle.create_exact(chart_id=chart_id, anchor_id="map_update", map_update=MapUpdateCert(
        n_active_tiles=n_active, tile_ids_active=list(keys), n_inactive_tiles=len(inactive),
        tile_ids_inactive=inactive, tile_cache_hits=hits, tile_cache_misses=len(active) - hits,
        candidate_tiles_per_meas_mean=float(mb.get("candidate_tiles_per_meas_mean", 0.0)),
        candidate_primitives_per_meas_mean=float(mb.get("candidate_primitives_per_meas_mean", 0.0)),
        candidate_primitives_per_meas_p95=float(mb.get("candidate_primitives_per_meas_p95", 0.0)),
        insert_count_total=n_inserted, insert_mass_total=mass_total, insert_mass_p95=mass_p95,
        evicted_count=n_culled, evicted_mass_total=evicted, fused_count=n_fused,
        fused_mass_total=float(stats[0]), merged_count=n_merged,
        staleness_inflation_strength=float(mb.get("staleness_inflation_strength", 0.0)),
        staleness_cov_inflation_trace=float(mb.get("staleness_cov_inflation_trace", 0.0)),
        stale_precision_downscale_total=float(mb.get("stale_precision_downscale_total", 0.0))))
    return result, cert, ExpectedEffect(objective_name="primitive_map_update", predicted=float(n_active * k_ins),
                                        realized=float(n_inserted))
