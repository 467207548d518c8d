// gc_camrender.hip — the camera view of the device map: what the reference's viewer
// (tools/view_splat_jaxsplat.py) does with the exported map and the last pose, with the raster it
// leaves to jaxsplat.render_v2 defined by this build ("Camera view").
//
//   gc_camera_splat_prep   per (view, primitive): cam_project (gc_renderdev.h: p = R mu + t, the pinhole
//                          mean, M at clamped tangents), the pushforward M Sigma M^T, its closed-form
//                          inverse and 3-sigma radius, the depth, the vMF shading towards the camera
//                          centre; per primitive alpha = clip(mass / m_max, alpha_floor, 1)
//                          (view_splat_jaxsplat.py:108-111), m_max reduced on the device.
//   gc_render_depth_tiles  per (view, tile): the cap nearest survivors of the bbox test by
//                          (depth, index) through the LDS selection the BEV lists use
//                          (gc_renderdev.h), then front-to-back compositing (its step: cam_step_alpha,
//                          cam_step_through there, shared with the depth evidence): one workgroup per tile,
//                          the tile's records staged in LDS, every lane reading the same record per step,
//                          each pixel's transmittance, colour, depth and count in registers in list order.
//
// Every sum runs in list order and nothing is accumulated with atomics except the mass maximum (an
// integer maximum, exact in any order): the outputs are bitwise reproducible from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"
#include "gc_renderdev.h"

namespace gc {
namespace {

constexpr int kCamRec = 12;   // a record: mean 2, Sigma^-1 4, alpha, rgb 3, depth, one pad (16-B aligned records)

// ------------------------------------------------------------------------------------------------
// splat preparation
// ------------------------------------------------------------------------------------------------

// The largest positive mass as the bits of a double: among positive doubles the unsigned integer order
// is the numeric order, so an integer maximum in any order is the exact maximum. *word starts at 0
// (no positive mass seen). At most kCamMaxBlocks workgroups stride over the rows, so one address takes at
// most 4 kCamMaxBlocks atomics.
constexpr int kCamMaxBlocks = 64;

__global__ __launch_bounds__(kRdT) void k_cam_mass_max(int64_t n, const double* mass, unsigned long long* word) {
  double x = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kRdT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRdT) {
    const double m = mass[i];
    x = m > x ? m : x;  // a NaN or a mass <= 0 does not count
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off, 64));
  if ((threadIdx.x & 63) == 0 && x > 0.0) atomicMax(word, (unsigned long long)__double_as_longlong(x));
}

// views v0 .. v0 + n_views - 1 (n_views <= kCamViewsPerLaunch), one lane per (view, primitive)
__global__ __launch_bounds__(kRdT) void k_cam_prep(int64_t n, int v0, int n_views, gc_render_batch b, CamViews views,
                                                   CamCfg c, const unsigned long long* mass_max, gc_cam_splats out) {
  const int64_t gl = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (gl >= n * n_views) return;
  const int vl = (int)(gl / n);
  const int64_t i = gl - (int64_t)vl * n;
  const int v = v0 + vl;
  const int64_t g = (int64_t)v * n + i;
  const double* V = views.v + kCamView * vl;
  double mu[3], S[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) S[q] = b.Sigma_world[9 * i + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) mu[q] = b.mu_world[3 * i + q];
  if (v == 0) {  // alpha is the primitive's, the same for every view
    const unsigned long long mw = *mass_max;
    const double m_max = mw ? __longlong_as_double((long long)mw) : 1.0;
    out.alphas[i] = fmin(fmax(b.mass[i] / m_max, c.alpha_floor), 1.0);
  }
  CamProj P;
  cam_project(V, mu, S, P);
  const double *p = P.p, *M = P.M, *MS = P.MS;
  bool ok = fabs(p[0]) < HUGE_VAL && fabs(p[1]) < HUGE_VAL && fabs(p[2]) < HUGE_VAL;
#pragma unroll
  for (int q = 0; q < 9; ++q) ok = ok && fabs(S[q]) < HUGE_VAL;
  ok = ok && p[2] > c.near && p[2] < c.far;
  if (!ok) {
    out.means_px[2 * g] = out.means_px[2 * g + 1] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) out.Sigmas_inv[4 * g + q] = 0.0;
    out.depths[g] = HUGE_VAL;
    out.radii[g] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) out.colors[3 * g + q] = 0.0;
    out.valid[g] = 0;
    return;
  }
  double Sp[4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 2; ++k) Sp[2 * r + k] = MS[3 * r] * M[3 * k] + MS[3 * r + 1] * M[3 * k + 1] + MS[3 * r + 2] * M[3 * k + 2];
  const double a = Sp[0] + c.lowpass, d = Sp[3] + c.lowpass, bb = 0.5 * (Sp[1] + Sp[2]);
  const double det = a * d - bb * bb;
  out.means_px[2 * g] = P.px;
  out.means_px[2 * g + 1] = P.py;
  out.Sigmas_inv[4 * g] = d / det;
  out.Sigmas_inv[4 * g + 1] = -bb / det;
  out.Sigmas_inv[4 * g + 2] = -bb / det;
  out.Sigmas_inv[4 * g + 3] = a / det;
  out.depths[g] = p[2];
  out.radii[g] = c.radius_sigma * sqrt(rd_eig_max2(a, bb, d));
  double s = 1.0;
  if (c.shade) {  // towards the camera centre
    const double vd[3] = {V[kCvCentre] - mu[0], V[kCvCentre + 1] - mu[1], V[kCvCentre + 2] - mu[2]};
    s = rd_vmf_shading(b.eta, i, b.n_lobes, vd);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) out.colors[3 * g + q] = b.color[3 * i + q] * s;
  out.valid[g] = 1;
}

// ------------------------------------------------------------------------------------------------
// tile lists: the cap nearest survivors by (depth, index)
// ------------------------------------------------------------------------------------------------

// depth where the splat is valid and its radius-r box meets the tile (all four strict), else +inf
struct CamKey {
  const double *means, *depths, *radii;
  const uint8_t* valid;
  double x0, y0, x1, y1;
  GC_DEV double operator()(int64_t i) const {
    const double mx = means[2 * i], my = means[2 * i + 1], r = radii[i];
    const bool in = valid[i] != 0 && mx + r > x0 && mx - r < x1 && my + r > y0 && my - r < y1;
    return in ? depths[i] : HUGE_VAL;
  }
};

__global__ __launch_bounds__(kRdT) void k_cam_bin_select(int64_t n, TileGrid G, const double* means, const double* depths,
                                                         const double* radii, const uint8_t* valid, int cap,
                                                         int32_t* counts, int32_t* survivors, int32_t* indices) {
  const int64_t seg = blockIdx.x;
  int ox, oy;
  const int64_t v = rd_seg_tile(seg, G, ox, oy);
  CamKey key;
  key.means = means + 2 * v * n;
  key.depths = depths + v * n;
  key.radii = radii + v * n;
  key.valid = valid + v * n;
  key.x0 = (double)ox;
  key.y0 = (double)oy;
  key.x1 = key.x0 + (double)G.ts;
  key.y1 = key.y0 + (double)G.ts;
  rd_select_smallest<true>(n, seg, key, cap, counts, survivors, indices);
}

// ------------------------------------------------------------------------------------------------
// front-to-back compositing
// ------------------------------------------------------------------------------------------------

struct CamRasterArgs {
  int64_t n;  // splats per view
  TileGrid G;
  int H, W, cap;
  const double *means, *Sinv, *alphas, *colors, *depths;
  const int32_t *indices, *counts;  // per segment cap entries; the count (<= cap <= kRdMaxCap)
  CamCfg c;
  double *images, *alpha, *depth;
  int32_t* n_contrib;
};

// One workgroup per (view, tile). The tile's list (at most kRdMaxCap records) is staged in LDS once;
// every lane reads the same record per step (identical addresses broadcast: no bank conflict). Thread
// t owns pixels t, t + 256, t + 512, t + 768 of the row-major tile and keeps T, C, D, n and a stopped
// flag for each in registers. A wave leaves the list loop once all of its pixels have stopped; there is
// one stage and so no barrier after the loop's start, which makes the wave the unit that can leave.
__global__ __launch_bounds__(kRdT) void k_cam_raster(CamRasterArgs A) {
  __shared__ double rec[kRdMaxCap * kCamRec];
  const int64_t seg = blockIdx.x;
  const int ts = A.G.ts;
  int ox, oy;
  const int64_t v = rd_seg_tile(seg, A.G, ox, oy);
  const int m = rd_clamp_count(A.counts[seg], A.cap);  // A.cap <= kRdMaxCap (the entry checks it)
  constexpr int kPix = kRdMaxTile * kRdMaxTile / kRdT;
  const int nk = (ts * ts + kRdT - 1) / kRdT;  // pixel slots in use (1 at tile_size 16): the rest are skipped
  double px[kPix], py[kPix], C[kPix][3], D[kPix], Tr[kPix];
  int cnt[kPix];
  bool live[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const int p = threadIdx.x + k * kRdT;
    px[k] = (double)(ox + p % ts) + 0.5;
    py[k] = (double)(oy + p / ts) + 0.5;
    C[k][0] = C[k][1] = C[k][2] = 0.0;
    D[k] = 0.0;
    Tr[k] = 1.0;
    cnt[k] = 0;
    live[k] = p < ts * ts;
  }
  if ((int)threadIdx.x < m) {
    const int64_t i = rd_list_index(A.indices[seg * A.cap + threadIdx.x], A.n);
    const int64_t r = v * A.n + i;
    double* o = rec + kCamRec * threadIdx.x;
    o[0] = A.means[2 * r];
    o[1] = A.means[2 * r + 1];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[2 + q] = A.Sinv[4 * r + q];
    o[6] = A.alphas[i];
#pragma unroll
    for (int q = 0; q < 3; ++q) o[7 + q] = A.colors[3 * r + q];
    o[10] = A.depths[r];
    o[11] = 0.0;
  }
  __syncthreads();
  for (int j = 0; j < m; ++j) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < kPix; ++k) any = any || live[k];
    if (!__any(any)) break;  // wave-uniform: every pixel of this wave has stopped
    const double* o = rec + kCamRec * j;
    const double mx = o[0], my = o[1], s00 = o[2], s01 = o[3], s10 = o[4], s11 = o[5], al = o[6];
    const double c0 = o[7], c1 = o[8], c2 = o[9], dep = o[10];
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      if (k >= nk) break;  // workgroup-uniform
      const double d0 = px[k] - mx, d1 = py[k] - my;
      double raw, a;
      cam_step_alpha(al, rd_quad(d0, d1, s00, s01, s10, s11), A.c.alpha_max, raw, a);
      if (live[k] && a >= A.c.alpha_skip) {
        const double w = Tr[k] * a;
        C[k][0] += w * c0;
        C[k][1] += w * c1;
        C[k][2] += w * c2;
        D[k] += w * dep;
        cnt[k] += 1;
        if (cam_step_through(Tr[k], a, A.c.t_stop)) live[k] = false;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const int p = threadIdx.x + k * kRdT;
    if (p >= ts * ts) continue;
    const int64_t row = (oy - A.G.oy0) + p / ts, col = (ox - A.G.ox0) + p % ts;
    const int64_t at = (v * A.H + row) * A.W + col;
#pragma unroll
    for (int q = 0; q < 3; ++q) A.images[3 * at + q] = C[k][q] + Tr[k] * A.c.bg[q];
    const double cover = 1.0 - Tr[k];
    A.alpha[at] = cover;
    A.depth[at] = cover > A.c.eps ? D[k] / cover : 0.0;
    A.n_contrib[at] = cnt[k];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_camera_splat_prep(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_views, const double* h_T_cw,
                             const double* h_intrinsics, int32_t H, int32_t W, const gc_camview_cfg* cfg,
                             const gc_cam_splats* out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, batch && h_T_cw && h_intrinsics && cfg && out, "NULL argument");
  GC_CHECK_ARG(ctx, n >= 0 && n <= ((int64_t)1 << 24), "n must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, n_views >= 1 && n_views <= kRdMaxViews, "n_views must be in [1, 32]");
  GC_CHECK_ARG(ctx, batch->n_lobes >= 1 && batch->n_lobes <= kMapMaxLobes, "n_lobes must be in [1, 8]");
  CamCfg c;
  if (int rc = cam_cfg(ctx, cfg, &c)) return rc;
  double hv[kRdMaxViews * kCamView];
  if (int rc = cam_pack_views(ctx, n_views, h_T_cw, h_intrinsics, nullptr, H, W, hv)) return rc;
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, batch->mu_world && batch->Sigma_world && batch->eta && batch->mass && batch->color, "NULL batch field");
  GC_CHECK_ARG(ctx, out->means_px && out->Sigmas_inv && out->depths && out->radii && out->alphas && out->colors && out->valid,
               "NULL output field");
  unsigned long long* word;
  if (int rc = carve_scratch(ctx, [&](Carver& cv) { word = cv.take<unsigned long long>(1); })) return rc;
  hipStream_t st = ctx->stream;
  GC_HIP(ctx, hipMemsetAsync(word, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_cam_mass_max, dim3(rd_blocks(n) < kCamMaxBlocks ? rd_blocks(n) : kCamMaxBlocks), dim3(kRdT), 0, st, n,
                     (const double*)batch->mass, word);
  GC_LAUNCH_CHECK(ctx);
  return cam_each_launch(ctx, n_views, hv, [&](int v0, int nv, const CamViews& views) {
    hipLaunchKernelGGL(k_cam_prep, dim3(rd_blocks(n * nv)), dim3(kRdT), 0, st, n, v0, nv, *batch, views, c,
                       (const unsigned long long*)word, *out);
  });
}

int32_t gc_render_depth_tiles(gc_ctx* ctx, int32_t n_views, int64_t n, const gc_cam_splats* splats, int32_t H, int32_t W,
                              int32_t tile_size, int32_t cap, const gc_camview_cfg* cfg, double* d_images,
                              double* d_alpha, double* d_depth, int32_t* d_n_contrib, int32_t* d_tile_counts,
                              int32_t* d_tile_survivors, int32_t* d_tile_indices) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  TileGrid G;
  int64_t segs;
  if (int rc = rd_tile_grid(ctx, n_views, n, H, W, tile_size, kRdMaxTile, cap,
                            {"n_views must be in [1, 32]", "tile_size must be in [1, 32]", "H and W must be in [1, 16384]",
                             "H and W must be multiples of tile_size", "n_views * tiles * n must be below 2^32"},
                            &G, &segs))
    return rc;
  CamRasterArgs A;
  if (int rc = cam_cfg(ctx, cfg, &A.c)) return rc;
  GC_CHECK_ARG(ctx, d_images && d_alpha && d_depth && d_n_contrib && d_tile_counts && d_tile_survivors && d_tile_indices,
               "NULL output buffer");
  hipStream_t st = ctx->stream;
  if (n == 0) {  // empty lists from memsets; the raster over them writes the background
    GC_HIP(ctx, hipMemsetAsync(d_tile_counts, 0, sizeof(int32_t) * (size_t)segs, st));
    GC_HIP(ctx, hipMemsetAsync(d_tile_survivors, 0, sizeof(int32_t) * (size_t)segs, st));
    GC_HIP(ctx, hipMemsetAsync(d_tile_indices, 0xFF, sizeof(int32_t) * (size_t)segs * cap, st));
    A.means = A.Sinv = A.alphas = A.colors = A.depths = nullptr;
  } else {
    GC_CHECK_ARG(ctx, splats && splats->means_px && splats->Sigmas_inv && splats->depths && splats->radii &&
                          splats->alphas && splats->colors && splats->valid, "NULL splat field");
    hipLaunchKernelGGL(k_cam_bin_select, dim3((unsigned)segs), dim3(kRdT), 0, st, n, G, (const double*)splats->means_px,
                       (const double*)splats->depths, (const double*)splats->radii, (const uint8_t*)splats->valid, (int)cap,
                       d_tile_counts, d_tile_survivors, d_tile_indices);
    GC_LAUNCH_CHECK(ctx);
    A.means = splats->means_px; A.Sinv = splats->Sigmas_inv; A.alphas = splats->alphas; A.colors = splats->colors;
    A.depths = splats->depths;
  }
  A.n = n; A.G = G; A.H = H; A.W = W; A.cap = cap;
  A.indices = d_tile_indices; A.counts = d_tile_counts;
  A.images = d_images; A.alpha = d_alpha; A.depth = d_depth; A.n_contrib = d_n_contrib;
  hipLaunchKernelGGL(k_cam_raster, dim3((unsigned)segs), dim3(kRdT), 0, st, A);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
