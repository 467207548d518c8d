"""Deterministic MA-hex 3D tiling on the host (common/tiling.py): world xyz -> cell (c1, c2, cz) ->
packed tile key, and the stencil enumeration that names the active and view tiles of a scan.

  c1 = floor(x / h), c2 = floor((x / 2 + y sqrt(3) / 2) / h), cz = floor(z / h)        (:32-63, :126-139)
  key = ((c1 + 2^20) & m) << 42 | ((c2 + 2^20) & m) << 21 | ((cz + 2^20) & m), m = 2^21 - 1  (:71-105)

The same arithmetic runs on the device where an operator assigns tiles itself
(gc_associate_primitives_ot, gc_primitive_map_update). These are the host forms a caller needs to
build `stencil_tile_ids` / `active_tile_ids` (pipeline.py:802-823)."""

from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .association import _PACK_BIAS, _PACK_BITS, _PACK_MASK, tile_id_from_cell_3d  # noqa: F401 (re-export)

_SQRT3_HALF = float(np.sqrt(3.0) * 0.5)


def hex_disk_axial(radius: int) -> List[Tuple[int, int]]:
    """tiling.py:171-186: the axial (q, r) cells of a hex disk of the given radius (inclusive),
    sorted; 3 r (r + 1) + 1 of them."""
    r = int(radius)
    return sorted((q, s) for q in range(-r, r + 1) for s in range(max(-r, -q - r), min(r, -q + r) + 1))


def tile_cells_from_xyz_batch(xyz, h_tile: float) -> np.ndarray:
    """(N, 3) world positions -> (N, 3) int64 cells, by floor (negative coordinates round down)."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    h = max(float(h_tile), 1e-12)
    s = np.stack([p[:, 0], p[:, 0] * 0.5 + p[:, 1] * _SQRT3_HALF, p[:, 2]], axis=1)
    return np.floor(s / h).astype(np.int64)


def tile_ids_from_cells(c1, c2, cz) -> np.ndarray:
    """tiling.py:148-163: packed int64 keys of cell arrays."""
    u = [(np.asarray(c, np.int64) + _PACK_BIAS) & _PACK_MASK for c in (c1, c2, cz)]
    return (u[0] << (2 * _PACK_BITS)) | (u[1] << _PACK_BITS) | u[2]


def tile_ids_from_xyz_batch(xyz, h_tile: float) -> np.ndarray:
    """tiling.py:113-145: (N, 3) world positions -> (N,) packed int64 tile keys."""
    c = tile_cells_from_xyz_batch(xyz, h_tile)
    return tile_ids_from_cells(c[:, 0], c[:, 1], c[:, 2])


def ma_hex_stencil_tile_ids(center_xyz, h_tile: float, radius_xy: int, radius_z: int) -> List[int]:
    """tiling.py:189-209: the tile keys of the stencil around center_xyz, a hex disk in (c1, c2) times a
    symmetric slab in cz, ordered by increasing cz and then by the sorted disk."""
    c1, c2, cz = (int(v) for v in tile_cells_from_xyz_batch(np.asarray(center_xyz, np.float64).ravel()[:3], h_tile)[0])
    disk = hex_disk_axial(radius_xy)
    return [tile_id_from_cell_3d(c1 + dq, c2 + dr, cz + dz)
            for dz in range(-int(radius_z), int(radius_z) + 1) for dq, dr in disk]
