"""Rendering the device map: the reference's output side on the GPU.

- renderable_batch_from_view / publish_renderable: what PrimitiveMapPublisher.publish returns
  (backend/map_publisher.py:131-242): the RenderablePrimitiveBatch
  (backend/structures/primitive_map.py:454-471) of the map's valid primitives, newest first, resident
  in HBM (DeviceRenderableBatch);
- BEVPushforwardConfig, oblique_P_from_config, oblique_Ps_bev15, pushforward_gaussian_3d_to_2d
  (common/bev_pushforward.py) and SplatRenderingConfig, splat_indices_for_tile, render_tile_ewa,
  fbm_at_splat_positions (backend/rendering.py), with the reference's names and signatures;
- render_map_bev: batch -> 2D splats of every view -> tile lists -> images, in three device calls with
  no wait between them. The reference has the pieces but never composes them; the composition is this
  build's and is declared in DESIGN.md §4.

- CameraViewConfig, camera_from_world, camera_splat_prep, render_depth_tiles, render_map_camera: the
  map seen through a pinhole at a camera pose, what tools/view_splat_jaxsplat.py renders from the exported
  map and the last trajectory pose: perspective splats, per-tile lists in depth order, front-to-back
  compositing, with a depth image beside the colour image. The raster the viewer leaves to
  jaxsplat.render_v2 is this build's and is declared in DESIGN.md §4 ("Camera view").

All arithmetic runs in libgcslam (csrc/gc_render.hip, csrc/gc_camrender.hip; what they share with the depth
evidence is csrc/gc_renderdev.h); every argument error is
raised here before a device is asked for."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np

from . import _abi
from ._abi import GC_RENDER_MAX_CAP, GC_RENDER_MAX_TILE, GC_RENDER_MAX_VIEWS
from .association import DeviceMapView, extract_atlas_map_view
from .constants import GC_EPS_LIFT
from .ops.camera_splats import PinholeIntrinsics
from .primitive_map import DevicePrimitiveMap


# ---------------------------------------------------------------------------------------------
# configuration (the reference's fields and defaults)
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class BEVPushforwardConfig:
    """bev_pushforward.py:16-27."""
    oblique_phi_deg: float = 10.0
    n_views: int = 15
    phi_center_deg: float = 10.0
    phi_span_deg: float = 14.0


@dataclass(frozen=True)
class SplatRenderingConfig:
    """rendering.py:28-44. The three vmf_intensity_* / vmf_kappa_max fields are kept for the
    reference's interface; the map carries no intensity, so the shading runs without it."""
    tile_size: int = 32
    max_splats_per_tile: int = 64
    fbm_octaves: int = 5
    fbm_gain: float = 0.5
    opacity_gamma: float = 1.0
    logdet0: float = 0.0
    eps: float = 1e-12
    ewa_log_clip: float = 25.0
    alpha_min: float = 0.02
    vmf_intensity_scale: float = 0.5
    vmf_intensity_max: float = 255.0
    vmf_kappa_max: float = 100.0


@dataclass(frozen=True)
class Viewport:
    """Where the image lies in the BEV plane: pixel (row, column) centre (r + 0.5, c + 0.5) is the BEV
    point origin_xy + (c + 0.5, r + 0.5) / px_per_m."""
    origin_xy: Tuple[float, float]
    px_per_m: float
    height: int
    width: int


def _oblique_P(phi_deg: float) -> np.ndarray:
    """bev_pushforward.py:30-39."""
    phi = np.deg2rad(float(phi_deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(phi), np.sin(phi)]], dtype=np.float64)


def _oblique_view_dir(phi_deg: float) -> np.ndarray:
    """The null vector of P(phi): the direction the oblique view looks along."""
    phi = np.deg2rad(float(phi_deg))
    return np.array([0.0, -np.sin(phi), np.cos(phi)], dtype=np.float64)


def oblique_P_from_config(config: BEVPushforwardConfig) -> np.ndarray:
    """bev_pushforward.py:67-69."""
    return _oblique_P(config.oblique_phi_deg)


def _bev15_phis(config: BEVPushforwardConfig) -> np.ndarray:
    """bev_pushforward.py:78-86."""
    n = max(1, int(config.n_views))
    center, span = float(config.phi_center_deg), float(config.phi_span_deg)
    if n == 1:
        return np.array([center], dtype=np.float64)
    return center + np.linspace(-0.5, 0.5, n, dtype=np.float64) * span


def oblique_Ps_bev15(config: BEVPushforwardConfig) -> np.ndarray:
    """bev_pushforward.py:72-88: (n_views, 2, 3)."""
    return np.stack([_oblique_P(phi) for phi in _bev15_phis(config)], axis=0)


# ---------------------------------------------------------------------------------------------
# renderable batch
# ---------------------------------------------------------------------------------------------

@dataclass
class RenderablePrimitiveBatch:
    """primitive_map.py:454-471, with the recency the rows are ordered by."""
    mu_world: np.ndarray
    Sigma_world: Optional[np.ndarray]
    Lambda_world: Optional[np.ndarray]
    eta: np.ndarray
    mass: np.ndarray
    color: np.ndarray
    primitive_ids: Optional[np.ndarray] = None
    last_supported_scan_seq: Optional[np.ndarray] = None


_BatchStruct = _abi.STRUCTS["gc_render_batch"]  # n_lobes, pad_, then the arrays of _BATCH_SHAPES
_SplatStruct = _abi.STRUCTS["gc_bev_splats"]


_BATCH_SHAPES = dict(mu_world=((3,), np.float64), Sigma_world=((3, 3), np.float64), Lambda_world=((3, 3), np.float64),
                     eta=None, mass=((), np.float64), color=((3,), np.float64), primitive_ids=((), np.int64),
                     last_supported_scan_seq=((), np.int64))


class DeviceRenderableBatch:
    """A RenderablePrimitiveBatch resident in HBM: `arrays` hold `capacity` rows each, the first
    `count` are the batch (newest first), the rest zero. download() gives the `count` rows."""

    def __init__(self, ctx, capacity: int, n_lobes: int):
        self.ctx, self.capacity, self.n_lobes, self.count = ctx, int(capacity), int(n_lobes), 0
        specs = [((self.capacity,) + ((self.n_lobes, 3) if v is None else v[0]), np.float64 if v is None else v[1])
                 for v in _BATCH_SHAPES.values()]
        self.arrays: Dict[str, _abi.DeviceArray] = dict(zip(_BATCH_SHAPES, _abi.alloc_many(ctx, specs)))
        self.struct = _BatchStruct(self.n_lobes, 0, *[self.arrays[k].ptr for k in _BATCH_SHAPES])

    @classmethod
    def from_host(cls, ctx, batch: RenderablePrimitiveBatch) -> "DeviceRenderableBatch":
        """Uploads a host batch (Sigma_world is required; a missing Lambda_world stays zero: the
        renderer does not read it)."""
        mu = np.ascontiguousarray(batch.mu_world, np.float64).reshape(-1, 3)
        n = mu.shape[0]
        if batch.Sigma_world is None:
            raise ValueError("the batch holds no Sigma_world")
        eta = np.ascontiguousarray(batch.eta, np.float64)
        if eta.ndim != 3 or eta.shape[0] != n or eta.shape[2] != 3 or not 1 <= eta.shape[1] <= 8:
            raise ValueError(f"eta of shape {eta.shape}, expected ({n}, 1..8, 3)")
        out = cls(ctx, n, eta.shape[1])
        out.count = n
        host = dict(mu_world=mu, Sigma_world=batch.Sigma_world, Lambda_world=batch.Lambda_world, eta=eta,
                    mass=batch.mass, color=batch.color, primitive_ids=batch.primitive_ids,
                    last_supported_scan_seq=batch.last_supported_scan_seq)
        for k, d in out.arrays.items():
            if host[k] is None:
                d.zero()
                continue
            a = np.asarray(host[k])
            if a.size != math.prod(d.shape):
                raise ValueError(f"{k} of shape {a.shape}, expected {d.shape}")
            if n:
                d.upload(a.reshape(d.shape))
        return out

    def download(self) -> RenderablePrimitiveBatch:
        host = _abi.download_many(list(self.arrays.values()))
        return RenderablePrimitiveBatch(**{k: np.ascontiguousarray(a[:self.count]) for k, a in zip(self.arrays, host)})


def renderable_batch_from_view(view: DeviceMapView, eps_lift: float = GC_EPS_LIFT) -> DeviceRenderableBatch:
    """map_publisher.py:143-242 from a DeviceMapView: its valid entries in the order
    np.lexsort((primitive_ids, -last_supported_scan_seq)) (newest first, ties by ascending primitive
    id), with Lambda_world = inv(Sigma_world + eps_lift I). One wait, for the count."""
    if math.isnan(float(eps_lift)):
        raise ValueError("eps_lift is NaN")
    out = DeviceRenderableBatch(view.ctx, view.count, view.n_lobes)
    n = C.c_int64(0)
    _abi.call("gc_renderable_batch_from_view", view.ctx.handle, C.byref(view.struct), float(eps_lift),
              C.byref(out.struct), C.byref(n), ctx=view.ctx)
    out.count = int(n.value)
    return out


def publish_renderable(atlas_map: DevicePrimitiveMap, tile_ids: Optional[Sequence[int]] = None,
                       max_primitives: Optional[int] = None, eps_lift: float = GC_EPS_LIFT) -> DeviceRenderableBatch:
    """PrimitiveMapPublisher.publish (map_publisher.py:131-242) without the ROS messages: the
    renderable batch of the listed tiles (default: every resident tile, sorted(atlas_map.tile_keys),
    as the reference takes sorted(primitive_map.tile_ids); a key that is not resident is an empty
    tile for the view, so a tile of the host store, stored_keys(), is published after ensure_tiles
    brought it in). max_primitives bounds the primitives taken per tile (default: m_tile, all of them).
    When it cuts a tile the selection is the view's (extract_atlas_map_view: by descending weight,
    ties by slot, over all slots); the reference's per-tile argsort(-w) over the valid slots breaks
    weight ties by slot order too, so the two agree wherever the weights at the cut are distinct."""
    if tile_ids is None:
        tile_ids = sorted(atlas_map.tile_keys)
    k = atlas_map.m_tile if max_primitives is None else int(max_primitives)
    if not 1 <= k <= atlas_map.m_tile:
        raise ValueError(f"max_primitives must be in [1, m_tile = {atlas_map.m_tile}], got {max_primitives}")
    tile_ids = [int(t) for t in tile_ids]
    if not tile_ids:
        return DeviceRenderableBatch(atlas_map.ctx, 0, atlas_map.n_lobes)
    return renderable_batch_from_view(extract_atlas_map_view(atlas_map, tile_ids, k, eps_lift=eps_lift), eps_lift)


def _device_batch(batch_or_map, ctx) -> DeviceRenderableBatch:
    """What the composed calls render: a device batch as it is, a map through publish_renderable, a host
    batch uploaded to ctx (None: the default context)."""
    if isinstance(batch_or_map, DevicePrimitiveMap):
        return publish_renderable(batch_or_map)
    if isinstance(batch_or_map, DeviceRenderableBatch):
        return batch_or_map
    if isinstance(batch_or_map, RenderablePrimitiveBatch):
        return DeviceRenderableBatch.from_host(ctx or _abi.default_context(), batch_or_map)
    raise ValueError(f"cannot render a {type(batch_or_map).__name__}")


# ---------------------------------------------------------------------------------------------
# BEV splats and the tile raster
# ---------------------------------------------------------------------------------------------

@dataclass
class BevRender:
    """render_map_bev's result: images (n_views, H, W, 3), the per-tile lists tile_counts
    (n_views, T) and tile_indices (n_views, T, cap; -1 past the count; T row-major tiles), and
    `device`, the DeviceArrays behind them and the 2D splats (means_px, Sigmas_inv, alphas, colors,
    fbm)."""
    images: np.ndarray
    tile_counts: np.ndarray
    tile_indices: np.ndarray
    device: Dict[str, _abi.DeviceArray]


def _check_raster_args(tile_size, height, width, cap, n) -> None:
    if int(tile_size) != tile_size or not 1 <= tile_size <= GC_RENDER_MAX_TILE:
        raise ValueError(f"tile_size must be an integer in [1, {GC_RENDER_MAX_TILE}], got {tile_size}")
    for what, v in (("height", height), ("width", width)):
        if int(v) != v or not 1 <= v <= 16384 or v % int(tile_size):
            raise ValueError(f"{what} must be a multiple of tile_size = {tile_size} in [1, 16384], got {v}")
    if int(cap) != cap or not 1 <= cap <= GC_RENDER_MAX_CAP:
        raise ValueError(f"max_splats_per_tile must be an integer in [1, {GC_RENDER_MAX_CAP}], got {cap}")
    if n < 0:
        raise ValueError(f"a negative splat count {n}")


def _bev_cfg(viewport: Viewport, cfg: SplatRenderingConfig, fbm_seed, fbm_modulate_scale):
    ox, oy = viewport.origin_xy
    h = _abi.cfg("gc_bev_cfg", cfg, origin_x=ox, origin_y=oy, px_per_m=viewport.px_per_m, fbm_seed=fbm_seed,
                 fbm_modulate_scale=fbm_modulate_scale)
    if not np.isfinite(np.frombuffer(h, np.float64)).all():
        raise ValueError("the viewport and the rendering configuration must be finite")
    if not viewport.px_per_m > 0.0:
        raise ValueError(f"px_per_m must be > 0, got {viewport.px_per_m}")
    if int(cfg.fbm_octaves) != cfg.fbm_octaves or not 0 <= cfg.fbm_octaves <= 32:
        raise ValueError(f"fbm_octaves must be an integer in [0, 32], got {cfg.fbm_octaves}")
    if int(fbm_seed) != fbm_seed or not 0 <= fbm_seed < 1 << 31:
        raise ValueError(f"fbm_seed must be an integer in [0, 2^31), got {fbm_seed}")
    return h


def bev_views(bev_cfg: BEVPushforwardConfig, views: str) -> Tuple[np.ndarray, np.ndarray]:
    """(P (n_views, 2, 3), view_dirs (n_views, 3)) of views = "bev15" (oblique_Ps_bev15) or "single"
    (oblique_P_from_config); view_dir is the null vector of P(phi), (0, -sin phi, cos phi)."""
    if views == "bev15":
        phis = _bev15_phis(bev_cfg)
    elif views == "single":
        phis = np.array([float(bev_cfg.oblique_phi_deg)], np.float64)
    else:
        raise ValueError(f'views must be "bev15" or "single", got {views!r}')
    if phis.shape[0] > GC_RENDER_MAX_VIEWS:
        raise ValueError(f"{phis.shape[0]} views; at most {GC_RENDER_MAX_VIEWS} are supported")
    return (np.stack([_oblique_P(p) for p in phis], axis=0), np.stack([_oblique_view_dir(p) for p in phis], axis=0))


def bev_splat_prep(batch: DeviceRenderableBatch, viewport: Viewport, P, view_dirs,
                   render_cfg: Optional[SplatRenderingConfig] = None, *, fbm_seed: int = 0,
                   fbm_modulate_scale: float = 0.0, with_sigma_bev: bool = False) -> Dict[str, _abi.DeviceArray]:
    """The 2D splats of the batch's `count` rows for every view (gc_bev_splat_prep, include/gcslam.h):
    means_px (n_views, n, 2), Sigmas_inv (n_views, n, 2, 2), alphas (n_views, n), colors
    (n_views, n, 3), fbm (n), and with with_sigma_bev Sigmas_bev (n_views, n, 2, 2). No wait."""
    cfg = render_cfg or SplatRenderingConfig()
    c_cfg = _bev_cfg(viewport, cfg, fbm_seed, fbm_modulate_scale)
    P = np.ascontiguousarray(P, np.float64)
    if P.ndim == 2:
        P = P[None]
    vd = np.ascontiguousarray(view_dirs, np.float64).reshape(-1, 3)
    nv = P.shape[0]
    if P.shape[1:] != (2, 3) or vd.shape[0] != nv or not 1 <= nv <= GC_RENDER_MAX_VIEWS:
        raise ValueError(f"P of shape {P.shape} and view_dirs of shape {vd.shape}: expected (n, 2, 3) and (n, 3), "
                         f"1 <= n <= {GC_RENDER_MAX_VIEWS}")
    if not (np.isfinite(P).all() and np.isfinite(vd).all()):
        raise ValueError("P and view_dirs must be finite")
    n, ctx = batch.count, batch.ctx
    names = ["means_px", "Sigmas_inv", "alphas", "colors", "fbm"] + (["Sigmas_bev"] if with_sigma_bev else [])
    shapes = dict(means_px=(nv, n, 2), Sigmas_inv=(nv, n, 2, 2), alphas=(nv, n), colors=(nv, n, 3), fbm=(n,),
                  Sigmas_bev=(nv, n, 2, 2))
    out = dict(zip(names, _abi.alloc_many(ctx, [shapes[k] for k in names])))
    st = _SplatStruct(*[out[k].ptr if k in out else None for k, _ in _SplatStruct._fields_])
    _abi.call("gc_bev_splat_prep", ctx.handle, C.byref(batch.struct), n, nv, P.ctypes.data, vd.ctypes.data,
              C.byref(c_cfg), C.byref(st), ctx=ctx)
    return out


def render_ewa_tiles(splats: Dict[str, _abi.DeviceArray], height: int, width: int, tile_size: int = 32,
                     max_splats_per_tile: int = 64, log_clip: float = 25.0, eps: float = 1e-12, *,
                     ctx=None) -> Dict[str, _abi.DeviceArray]:
    """Tile binning and EWA raster of 2D splats (gc_render_ewa_tiles): images (n_views, H, W, 3),
    tile_counts (n_views, T), tile_indices (n_views, T, cap), all on the device. No wait."""
    nv, n = splats["alphas"].shape
    _check_raster_args(tile_size, height, width, max_splats_per_tile, n)
    if math.isnan(float(log_clip)) or math.isnan(float(eps)):
        raise ValueError("log_clip or eps is NaN")
    ts, H, W, cap = int(tile_size), int(height), int(width), int(max_splats_per_tile)
    T = (H // ts) * (W // ts)
    if nv * T * n >= 1 << 32:
        raise ValueError(f"n_views * tiles * n = {nv * T * n} must be below 2^32")
    ctx = ctx or splats["alphas"].ctx
    img, cnt, idx = _abi.alloc_many(ctx, [((nv, H, W, 3), np.float64), ((nv, T), np.int32), ((nv, T, cap), np.int32)])
    st = _SplatStruct(*[splats[k].ptr if k in splats else None for k, _ in _SplatStruct._fields_])
    _abi.call("gc_render_ewa_tiles", ctx.handle, nv, n, C.byref(st), H, W, ts, cap, float(log_clip), float(eps),
              img.ptr, cnt.ptr, idx.ptr, ctx=ctx)
    return dict(images=img, tile_counts=cnt, tile_indices=idx)


def render_map_bev(batch_or_map: Union[DeviceRenderableBatch, RenderablePrimitiveBatch, DevicePrimitiveMap],
                   viewport: Viewport, render_cfg: Optional[SplatRenderingConfig] = None,
                   bev_cfg: Optional[BEVPushforwardConfig] = None, views: str = "bev15", *, fbm_seed: int = 0,
                   fbm_modulate_scale: float = 0.0, ctx=None) -> BevRender:
    """The BEV images of a renderable batch (or of a map: publish_renderable first). views = "bev15":
    the n_views oblique views of oblique_Ps_bev15; "single": the one of oblique_P_from_config. Per
    view, the batch's Gaussians are pushed forward with P, mapped to pixels by the viewport, given
    their opacity, shading and fBm colour (DESIGN.md §4 declares the composition), binned into
    tile_size x tile_size tiles of at most max_splats_per_tile splats and rastered
    (render_cfg: SplatRenderingConfig). fbm_modulate_scale and fbm_seed are render_tile_ewa's
    arguments of those names (rendering.py:309-310; 0: the colours are not modulated).
    ValueError before any launch for a tile_size outside [1, 32], a height or width that is no
    multiple of it, or max_splats_per_tile outside [1, 256]."""
    cfg, bcfg = render_cfg or SplatRenderingConfig(), bev_cfg or BEVPushforwardConfig()
    H, W = viewport.height, viewport.width
    _check_raster_args(cfg.tile_size, H, W, cfg.max_splats_per_tile, 0)
    _bev_cfg(viewport, cfg, fbm_seed, fbm_modulate_scale)
    P, vd = bev_views(bcfg, views)
    batch = _device_batch(batch_or_map, ctx)
    splats = bev_splat_prep(batch, viewport, P, vd, cfg, fbm_seed=fbm_seed, fbm_modulate_scale=fbm_modulate_scale)
    dev = render_ewa_tiles(splats, H, W, cfg.tile_size, cfg.max_splats_per_tile, cfg.ewa_log_clip, cfg.eps,
                           ctx=batch.ctx)
    images, counts, indices = _abi.download_many([dev["images"], dev["tile_counts"], dev["tile_indices"]])
    return BevRender(images=images.copy(), tile_counts=counts.copy(), tile_indices=indices.copy(),
                     device=dict(dev, **splats))


# ---------------------------------------------------------------------------------------------
# the camera view: perspective splats, depth-ordered lists, front-to-back compositing
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class CameraViewConfig:
    """The camera view's raster ("Camera view"). alpha_floor is the viewer's clip of
    mass / m_max (view_splat_jaxsplat.py:111); the rest is the build's."""
    tile_size: int = 16
    max_splats_per_tile: int = 256
    near: float = 0.2
    far: float = 100.0
    lowpass_px2: float = 0.3
    radius_sigma: float = 3.0
    alpha_floor: float = 0.01
    alpha_max: float = 0.99
    alpha_skip: float = 1.0 / 255.0
    t_stop: float = 1e-4
    background: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    shade: bool = True
    eps: float = 1e-12


@dataclass
class CameraRender:
    """render_map_camera's result: images (n_views, H, W, 3), alpha and depth (n_views, H, W), n_contrib
    (n_views, H, W) int32, the per-tile lists tile_counts and tile_survivors (n_views, T; the survivors
    before the cut at max_splats_per_tile), tile_indices (n_views, T, cap; -1 past the count), and
    `device`, the DeviceArrays behind them and the 2D splats."""
    images: np.ndarray
    alpha: np.ndarray
    depth: np.ndarray
    n_contrib: np.ndarray
    tile_counts: np.ndarray
    tile_survivors: np.ndarray
    tile_indices: np.ndarray
    device: Dict[str, _abi.DeviceArray]


_CamSplatStruct = _abi.STRUCTS["gc_cam_splats"]


def _extrinsics(R_base_camera, t_base_camera) -> Tuple[np.ndarray, np.ndarray]:
    """(R_bc (3, 3), t_bc (3,)), the camera at the body by default; the shapes are checked here, what else a
    caller requires of them by the caller."""
    Rbc = np.eye(3) if R_base_camera is None else np.asarray(R_base_camera, np.float64)
    tbc = np.zeros(3) if t_base_camera is None else np.asarray(t_base_camera, np.float64).reshape(-1)
    if Rbc.shape != (3, 3) or tbc.shape != (3,):
        raise ValueError(f"R_base_camera of shape {Rbc.shape} and t_base_camera of shape {tbc.shape}: expected (3, 3), (3,)")
    return Rbc, tbc


def camera_from_world(pose, R_base_camera=None, t_base_camera=None, *, ctx=None) -> np.ndarray:
    """T_cw = inv(T_wb T_bc) (4, 4): what the viewer takes as its camera (view_splat_jaxsplat.py:103,
    camera-at-body: T_bc = I, the default). pose is the body pose in the world, either the 6-vector
    (translation, rotation vector; the rotation through ops/se3.so3_exp, on the device) or a 4 x 4
    T_wb, which needs no device. P poses as (P, 6) or (P, 4, 4) give (P, 4, 4): one so3_exp call for the
    batch, and every T_cw the bytes of the single call for its pose."""
    p = np.asarray(pose, np.float64)
    Rbc, tbc = _extrinsics(R_base_camera, t_base_camera)
    if p.shape not in ((6,), (4, 4)) and not (p.ndim in (2, 3) and p.shape[1:] in ((6,), (4, 4))):
        raise ValueError(f"pose of shape {p.shape}: expected (6,) or (4, 4)")
    if not (np.isfinite(p).all() and np.isfinite(Rbc).all() and np.isfinite(tbc).all()):
        raise ValueError("the pose and the extrinsics must be finite")
    single = p.shape in ((6,), (4, 4))
    ps = p[None] if single else p
    if ps.shape[1:] == (4, 4):
        if not (ps[:, 3] == np.array([0.0, 0.0, 0.0, 1.0])).all():
            raise ValueError("the bottom row of T_wb must be (0, 0, 0, 1)")
        Rwb, twb = ps[:, :3, :3], ps[:, :3, 3]
    else:
        from .ops import se3
        Rwb, twb = np.asarray(se3.so3_exp(ps[:, 3:], ctx=ctx), np.float64).reshape(-1, 3, 3), ps[:, :3]
    T = np.tile(np.eye(4), (ps.shape[0], 1, 1))
    for i in range(ps.shape[0]):  # 3 x 3 products one pose at a time: the bytes do not depend on the batch
        Rwc, twc = Rwb[i] @ Rbc, Rwb[i] @ tbc + twb[i]
        T[i, :3, :3], T[i, :3, 3] = Rwc.T, -Rwc.T @ twc
    return T[0] if single else T


def _camview_cfg(cfg: CameraViewConfig):
    bg = np.asarray(cfg.background, np.float64).reshape(-1)
    if bg.shape != (3,):
        raise ValueError(f"background must hold 3 values, got {cfg.background!r}")
    h = _abi.cfg("gc_camview_cfg", cfg, bg_r=bg[0], bg_g=bg[1], bg_b=bg[2], shade=bool(cfg.shade))
    if not np.isfinite(np.frombuffer(h, np.float64)).all():
        raise ValueError("the camera view configuration must be finite")
    if not (cfg.near > 0.0 and cfg.far > cfg.near):
        raise ValueError(f"near must be > 0 and far > near, got near = {cfg.near}, far = {cfg.far}")
    if not 0.0 < cfg.alpha_max <= 1.0:
        raise ValueError(f"alpha_max must be in (0, 1], got {cfg.alpha_max}")
    return h


def _cam_views(intrinsics, T_cw) -> Tuple[np.ndarray, np.ndarray]:
    """(T_cw (n_views, 4, 4), intrinsics (n_views, 4) as fx fy cx cy), checked."""
    T = np.ascontiguousarray(T_cw, np.float64)
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError(f"T_cw of shape {np.shape(T_cw)}: expected (4, 4) or (n_views, 4, 4)")
    nv = T.shape[0]
    if not 1 <= nv <= GC_RENDER_MAX_VIEWS:
        raise ValueError(f"{nv} views; between 1 and {GC_RENDER_MAX_VIEWS} are supported")
    ks = [intrinsics] if isinstance(intrinsics, PinholeIntrinsics) else list(intrinsics)
    if len(ks) != nv:
        raise ValueError(f"{len(ks)} intrinsics for {nv} views")
    K = np.array([[k.fx, k.fy, k.cx, k.cy] for k in ks], np.float64).reshape(nv, 4)
    if not (np.isfinite(T).all() and np.isfinite(K).all()):
        raise ValueError("T_cw and the intrinsics must be finite")
    if not (K[:, :2] > 0.0).all():
        raise ValueError("fx and fy must be > 0")
    if not (T[:, 3] == np.array([0.0, 0.0, 0.0, 1.0])).all():
        raise ValueError("the bottom row of T_cw must be (0, 0, 0, 1)")
    R = T[:, :3, :3]
    if np.max(np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3))) > 1e-9:
        raise ValueError("the 3 x 3 block of T_cw must be a rotation (max |R^T R - I| <= 1e-9)")
    return T, K


def _check_camera_args(intrinsics, T_cw, height, width, cfg: CameraViewConfig, n: int):
    _check_raster_args(cfg.tile_size, height, width, cfg.max_splats_per_tile, n)
    c_cfg = _camview_cfg(cfg)
    T, K = _cam_views(intrinsics, T_cw)
    tiles = (int(height) // int(cfg.tile_size)) * (int(width) // int(cfg.tile_size))
    if T.shape[0] * tiles * n >= 1 << 32:
        raise ValueError(f"n_views * tiles * n = {T.shape[0] * tiles * n} must be below 2^32")
    return c_cfg, T, K


def camera_splat_prep(batch: DeviceRenderableBatch, intrinsics, T_cw, height: int, width: int,
                      cfg: Optional[CameraViewConfig] = None) -> Dict[str, _abi.DeviceArray]:
    """The 2D splats of the batch's `count` rows for every camera view (gc_camera_splat_prep,
    include/gcslam.h): means_px (n_views, n, 2), Sigmas_inv (n_views, n, 2, 2), depths and radii
    (n_views, n), alphas (n), colors (n_views, n, 3), valid (n_views, n) uint8. intrinsics: a
    PinholeIntrinsics or one per view; T_cw (4, 4) or (n_views, 4, 4) (camera_from_world). No wait."""
    cfg = cfg or CameraViewConfig()
    n, ctx = batch.count, batch.ctx
    c_cfg, T, K = _check_camera_args(intrinsics, T_cw, height, width, cfg, n)
    nv = T.shape[0]
    names = [k for k, _ in _CamSplatStruct._fields_]
    specs = dict(means_px=((nv, n, 2), np.float64), Sigmas_inv=((nv, n, 2, 2), np.float64), depths=((nv, n), np.float64),
                 radii=((nv, n), np.float64), alphas=((n,), np.float64), colors=((nv, n, 3), np.float64),
                 valid=((nv, n), np.uint8))
    out = dict(zip(names, _abi.alloc_many(ctx, [specs[k] for k in names])))
    st = _CamSplatStruct(*[out[k].ptr for k in names])
    _abi.call("gc_camera_splat_prep", ctx.handle, C.byref(batch.struct), n, nv, T.ctypes.data, K.ctypes.data, int(height),
              int(width), C.byref(c_cfg), C.byref(st), ctx=ctx)
    return out


def render_depth_tiles(splats: Dict[str, _abi.DeviceArray], height: int, width: int,
                       cfg: Optional[CameraViewConfig] = None, *, ctx=None) -> Dict[str, _abi.DeviceArray]:
    """The depth-ordered tile lists and the front-to-back composite of camera splats
    (gc_render_depth_tiles): images (n_views, H, W, 3), alpha, depth (n_views, H, W), n_contrib
    (n_views, H, W) int32, tile_counts, tile_survivors (n_views, T), tile_indices (n_views, T, cap),
    all on the device. No wait."""
    cfg = cfg or CameraViewConfig()
    nv, n = splats["depths"].shape
    _check_raster_args(cfg.tile_size, height, width, cfg.max_splats_per_tile, n)
    c_cfg = _camview_cfg(cfg)
    if not 1 <= nv <= GC_RENDER_MAX_VIEWS:
        raise ValueError(f"{nv} views; between 1 and {GC_RENDER_MAX_VIEWS} are supported")
    ts, H, W, cap = int(cfg.tile_size), int(height), int(width), int(cfg.max_splats_per_tile)
    T = (H // ts) * (W // ts)
    if nv * T * n >= 1 << 32:
        raise ValueError(f"n_views * tiles * n = {nv * T * n} must be below 2^32")
    ctx = ctx or splats["depths"].ctx
    names = ("images", "alpha", "depth", "n_contrib", "tile_counts", "tile_survivors", "tile_indices")
    arrays = _abi.alloc_many(ctx, [((nv, H, W, 3), np.float64), ((nv, H, W), np.float64), ((nv, H, W), np.float64),
                                   ((nv, H, W), np.int32), ((nv, T), np.int32), ((nv, T), np.int32),
                                   ((nv, T, cap), np.int32)])
    st = _CamSplatStruct(*[splats[k].ptr for k, _ in _CamSplatStruct._fields_])
    _abi.call("gc_render_depth_tiles", ctx.handle, nv, n, C.byref(st), H, W, ts, cap, C.byref(c_cfg),
              *[a.ptr for a in arrays], ctx=ctx)
    return dict(zip(names, arrays))


def render_map_camera(batch_or_map: Union[DeviceRenderableBatch, RenderablePrimitiveBatch, DevicePrimitiveMap],
                      intrinsics, T_cw, height: int, width: int, cfg: Optional[CameraViewConfig] = None, *,
                      ctx=None) -> CameraRender:
    """The map through a pinhole at T_cw (camera_from_world of the pose): colour, coverage and depth
    images of a renderable batch (or of a map: publish_renderable first), one per view. The two device
    calls run with no wait between them and everything is downloaded once at the end. ValueError
    before a device is asked for: see DESIGN.md §4 for the list."""
    cfg = cfg or CameraViewConfig()
    _check_camera_args(intrinsics, T_cw, height, width, cfg, 0)
    batch = _device_batch(batch_or_map, ctx)
    splats = camera_splat_prep(batch, intrinsics, T_cw, height, width, cfg)
    dev = render_depth_tiles(splats, height, width, cfg, ctx=batch.ctx)
    names = ("images", "alpha", "depth", "n_contrib", "tile_counts", "tile_survivors", "tile_indices")
    host = _abi.download_many([dev[k] for k in names])
    return CameraRender(**{k: a.copy() for k, a in zip(names, host)}, device=dict(dev, **splats))


# ---------------------------------------------------------------------------------------------
# drop-ins: the reference's functions, one tile (or one Gaussian) on the device
# ---------------------------------------------------------------------------------------------

def _clamp_tile(tile_size) -> int:
    return min(max(int(tile_size), 1), GC_RENDER_MAX_TILE)  # rendering.py:267, :320


def _origin(tile_origin) -> Tuple[int, int]:
    oy, ox = int(tile_origin[0]), int(tile_origin[1])
    if max(abs(oy), abs(ox)) > 1 << 24:
        raise ValueError(f"tile origin {tile_origin} outside [-2^24, 2^24]")
    return oy, ox


def splat_indices_for_tile(tile_origin, tile_size: int, means, Sigmas_inv, max_splats_per_tile: int = 64,
                           eps: float = 1e-12, *, ctx=None) -> np.ndarray:
    """rendering.py:252-289: the splats whose 2-sigma bbox meets the tile, nearest the tile centre
    first (ties by index), at most max_splats_per_tile of them."""
    oy, ox = _origin(tile_origin)
    ts = _clamp_tile(tile_size)
    N = np.shape(means)[0]
    if N == 0:
        return np.array([], dtype=np.int64)
    cap = int(max_splats_per_tile)
    if cap <= 0:
        return np.array([], dtype=np.int64)  # overlapping[:0]
    cap = min(cap, 1 << 24)
    if math.isnan(float(eps)):
        raise ValueError("eps is NaN")
    m = np.ascontiguousarray(means, np.float64).reshape(N, 2)
    S = np.ascontiguousarray(Sigmas_inv, np.float64).reshape(N, 2, 2)
    ctx = ctx or _abi.default_context()
    dm, dS = _abi.upload_many(ctx, [m, S])
    d_idx = _abi.DeviceArray(ctx, (min(cap, N),), np.int32)
    cnt = C.c_int32(0)
    _abi.call("gc_splat_indices_for_tile", ctx.handle, N, dm.ptr, dS.ptr, oy, ox, ts, cap, float(eps), d_idx.ptr,
              C.byref(cnt), ctx=ctx)
    return d_idx.download()[:int(cnt.value)].astype(np.int64)


def fbm_at_splat_positions(means_world_xy, octaves: int = 5, gain: float = 0.5, seed: int = 0, *, ctx=None) -> np.ndarray:
    """rendering.py:212-228: fBm value noise at each (x, y). The integer hash is the reference's while
    |coordinate| * 2^(octaves - 1) < 2^31; ValueError outside that domain."""
    xy = np.ascontiguousarray(means_world_xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    if int(octaves) != octaves or not 0 <= octaves <= 32:
        raise ValueError(f"octaves must be an integer in [0, 32], got {octaves}")
    if int(seed) != seed or not 0 <= seed < 1 << 31:
        raise ValueError(f"seed must be an integer in [0, 2^31), got {seed}")
    if math.isnan(float(gain)):
        raise ValueError("gain is NaN")
    if n == 0:
        return np.zeros(0, np.float64)
    if not np.isfinite(xy).all() or float(np.max(np.abs(xy))) * 2.0 ** max(int(octaves) - 1, 0) >= 2.0 ** 31:
        raise ValueError("a coordinate outside the hash's domain |coordinate| * 2^(octaves - 1) < 2^31")
    ctx = ctx or _abi.default_context()
    (dxy,) = _abi.upload_many(ctx, [xy])
    out = _abi.DeviceArray(ctx, (n,), np.float64)
    _abi.call("gc_fbm_at_positions", ctx.handle, n, dxy.ptr, int(octaves), float(gain), int(seed), out.ptr, ctx=ctx)
    return out.download()


def render_tile_ewa(tile_origin, tile_size: int, means, Sigmas_inv, alphas, colors, splat_indices=None,
                    log_clip: float = 25.0, means_world_xy=None, fbm_octaves: int = 5, fbm_gain: float = 0.5,
                    fbm_seed: int = 0, fbm_modulate_scale: float = 0.0, *, ctx=None) -> np.ndarray:
    """rendering.py:297-355: one tile_size x tile_size tile of EWA splats, RGB in [0, 1]. splat_indices
    (optional) restricts and orders the splats; with means_world_xy and fbm_modulate_scale > 0 the
    colours are modulated by the fBm at the world positions (computed on the device as well)."""
    oy, ox = _origin(tile_origin)
    ts = _clamp_tile(tile_size)
    N = np.shape(means)[0]
    if math.isnan(float(log_clip)):
        raise ValueError("log_clip is NaN")
    if N == 0:
        return np.zeros((ts, ts, 3), np.float64)
    idx = None
    if splat_indices is not None:
        idx = np.asarray(splat_indices).reshape(-1)
        if idx.size == 0:
            return np.zeros((ts, ts, 3), np.float64)
        idx = idx.astype(np.int64)
        if (idx < -N).any() or (idx >= N).any():
            raise IndexError(f"splat index outside [-{N}, {N})")
        idx = np.where(idx < 0, idx + N, idx).astype(np.int32)
    m = np.ascontiguousarray(means, np.float64).reshape(N, 2)
    S = np.ascontiguousarray(Sigmas_inv, np.float64).reshape(N, 2, 2)
    a = np.ascontiguousarray(alphas, np.float64).reshape(N)
    c = np.ascontiguousarray(np.asarray(colors, np.float64).reshape(-1, 3)[:N])
    ctx = ctx or _abi.default_context()
    if fbm_modulate_scale > 0.0 and means_world_xy is not None:  # :333-340
        world = np.asarray(means_world_xy, np.float64).reshape(-1, 2)[:N]
        f = fbm_at_splat_positions(world, octaves=fbm_octaves, gain=fbm_gain, seed=fbm_seed, ctx=ctx)
        c = c * ((1.0 - fbm_modulate_scale) + fbm_modulate_scale * f)[:, np.newaxis]
    dm, dS, da, dc = _abi.upload_many(ctx, [m, S, a, c])
    d_idx = _abi.DeviceArray.from_host(ctx, idx, np.int32) if idx is not None else None
    out = _abi.DeviceArray(ctx, (ts, ts, 3), np.float64)
    _abi.call("gc_render_tile_ewa", ctx.handle, N, dm.ptr, dS.ptr, da.ptr, dc.ptr, oy, ox, ts,
              d_idx.ptr if d_idx is not None else None, idx.shape[0] if idx is not None else -1, float(log_clip),
              out.ptr, ctx=ctx)
    return out.download()


def pushforward_gaussian_3d_to_2d(mu, Sigma, P, *, ctx=None) -> Tuple[np.ndarray, np.ndarray]:
    """bev_pushforward.py:42-64: (mu_bev (2,), Sigma_bev (2, 2)) = (P mu, P Sigma P^T), computed by the
    splat preparation with the identity pixel map."""
    mu = np.asarray(mu, dtype=np.float64).ravel()[:3]
    Sigma = np.asarray(Sigma, dtype=np.float64).reshape(3, 3)
    P = np.asarray(P, dtype=np.float64).reshape(2, 3)
    ctx = ctx or _abi.default_context()
    b = DeviceRenderableBatch.from_host(ctx, RenderablePrimitiveBatch(
        mu_world=mu[None], Sigma_world=Sigma[None], Lambda_world=None, eta=np.zeros((1, 1, 3)), mass=np.ones(1),
        color=np.zeros((1, 3))))
    s = bev_splat_prep(b, Viewport((0.0, 0.0), 1.0, 1, 1), P, np.array([0.0, 0.0, 1.0]), with_sigma_bev=True)
    return s["means_px"].download().reshape(2), s["Sigmas_bev"].download().reshape(2, 2)
