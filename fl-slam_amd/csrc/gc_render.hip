// gc_render.hip — the output side of the device PrimitiveMap: what the reference's per-scan loop ends
// with (backend/backend_node.py:2274-2285 -> backend/map_publisher.py:131-242) and what its renderer
// (backend/rendering.py, common/bev_pushforward.py) makes of the published batch.
//
//   gc_renderable_batch_from_view  the valid entries of a map view, newest first (ties by ascending
//                                  primitive id: np.lexsort((primitive_ids, -last_supported_scan_seq)),
//                                  map_publisher.py:200), compacted into a RenderablePrimitiveBatch with
//                                  Lambda_world = inv(Sigma_world + eps_lift I) (:232-233). Two stable
//                                  passes of gc::radix_sort_pairs: by id ascending, then by recency
//                                  descending.
//   gc_bev_splat_prep              per (view, splat): mu_bev = P mu, Sigma_bev = P Sigma P^T
//                                  (bev_pushforward.py:59-64), opacity_from_logdet (rendering.py:236-244),
//                                  vmf_shading_multi_lobe (:117-159), fbm_value_noise (:167-209) and the
//                                  colour modulation (:333-340), composed as DESIGN.md declares.
//   gc_render_ewa_tiles            splat_indices_for_tile (:252-289) for every (view, tile): one workgroup
//                                  scans the splats in index order and keeps the cap nearest survivors of
//                                  the bbox test by (dist_sq, index) in LDS; then render_tile_ewa
//                                  (:297-355): one workgroup per (view, tile), the tile's splat records
//                                  staged in LDS, every lane reading the same record per step, each
//                                  pixel's sums kept in registers in list order.
//   gc_splat_indices_for_tile, gc_render_tile_ewa, gc_fbm_at_positions
//                                  one tile / the noise alone, with the reference's own arguments (any
//                                  tile origin, any index list), through the same kernels.
//
// Every sum runs in a fixed order and nothing is accumulated with atomics except one integer count:
// the outputs are bitwise reproducible from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"
#include "gc_renderdev.h"
#include "gc_sort.h"

namespace gc {
namespace {

// kRdT, kRdMaxTile, kRdMaxCap and kRdMaxViews (9 doubles per view here): gc_renderdev.h
constexpr int kRdRec = 10;            // a record: mean 2, Sigma^-1 4, alpha 1, rgb 3

// ------------------------------------------------------------------------------------------------
// renderable batch
// ------------------------------------------------------------------------------------------------

// pass 1 keys: the primitive id (ascending), +inf where the entry is not valid; the number of valid entries
__global__ __launch_bounds__(kRdT) void k_rb_keys_id(int64_t V, const uint8_t* valid, const int64_t* pid, double* keys,
                                                     uint32_t* vals, int32_t* count) {
  const int64_t i = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  const bool ok = i < V && valid[i] != 0;
  if (i < V) {
    keys[i] = ok ? (double)pid[i] : HUGE_VAL;
    vals[i] = (uint32_t)i;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (int32_t)__popcll(m));
}

// pass 2 keys, in the order pass 1 left: the recency (descending), -inf where the entry is not valid
__global__ __launch_bounds__(kRdT) void k_rb_keys_seq(int64_t V, const uint8_t* valid, const int64_t* seq,
                                                      const uint32_t* order, double* keys) {
  const int64_t j = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (j >= V) return;
  const uint32_t i = order[j];
  keys[j] = valid[i] ? (double)seq[i] : -HUGE_VAL;
}

__global__ __launch_bounds__(kRdT) void k_rb_gather(int64_t V, gc_map_view view, const uint32_t* order,
                                                    const int32_t* count, double eps_lift, gc_render_batch out) {
  const int64_t j = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (j >= V) return;
  const int L = out.n_lobes;
  if (j < (int64_t)*count) {
    const int64_t i = order[j];
    double S[9], Sg[9], Lm[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      S[q] = view.covariances[9 * i + q];
      Sg[q] = S[q] + ((q % 4 == 0) ? eps_lift : 0.0);
    }
    inv3(Sg, Lm);
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      out.Sigma_world[9 * j + q] = S[q];
      out.Lambda_world[9 * j + q] = Lm[q];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      out.mu_world[3 * j + q] = view.positions[3 * i + q];
      out.color[3 * j + q] = view.colors[3 * i + q];
    }
    for (int q = 0; q < 3 * L; ++q) out.eta[3 * L * j + q] = view.etas[3 * L * i + q];
    out.mass[j] = view.weights[i];
    out.primitive_ids[j] = view.primitive_ids[i];
    out.last_supported_scan_seq[j] = view.last_supported_scan_seq[i];
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      out.Sigma_world[9 * j + q] = 0.0;
      out.Lambda_world[9 * j + q] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      out.mu_world[3 * j + q] = 0.0;
      out.color[3 * j + q] = 0.0;
    }
    for (int q = 0; q < 3 * L; ++q) out.eta[3 * L * j + q] = 0.0;
    out.mass[j] = 0.0;
    out.primitive_ids[j] = 0;
    out.last_supported_scan_seq[j] = 0;
  }
}

// ------------------------------------------------------------------------------------------------
// fBm value noise (rendering.py:167-209)
// ------------------------------------------------------------------------------------------------

// _hash_float (:167-170). h < 2^31, so the product stays below 2^62.
GC_DEV double rd_hash_float(int64_t h) {
  h = (h * 1103515245ll + 12345ll) & 0x7FFFFFFFll;
  return (double)h / 2147483648.0;
}

// The cell hash of _value_noise_2d (:180-183). Python masks an integer of any size; int64 two's
// complement gives the same low 31 bits, negative cells included, while nothing overflows:
// |seed * 961 + ix * 31 + iy| < 2^63, which |coordinate| * 2^(octaves - 1) < 2^31 guarantees.
GC_DEV double rd_cell(int64_t seed, int64_t ix, int64_t iy) {
  return rd_hash_float(((seed * 31 + ix) * 31 + iy) & 0x7FFFFFFFll);
}

// _value_noise_2d (:173-188)
GC_DEV double rd_value_noise(double x, double y, int64_t seed) {
  const double flx = floor(x), fly = floor(y);
  const int64_t ix = (int64_t)flx, iy = (int64_t)fly;
  double fx = x - flx, fy = y - fly;
  fx = fmax(0.0, fmin(1.0, fx));
  fy = fmax(0.0, fmin(1.0, fy));
  const double v00 = rd_cell(seed, ix, iy), v10 = rd_cell(seed, ix + 1, iy);
  const double v01 = rd_cell(seed, ix, iy + 1), v11 = rd_cell(seed, ix + 1, iy + 1);
  const double sx = fx * fx * (3.0 - 2.0 * fx), sy = fy * fy * (3.0 - 2.0 * fy);
  const double v0 = v00 * (1.0 - sx) + v10 * sx;
  const double v1 = v01 * (1.0 - sx) + v11 * sx;
  return v0 * (1.0 - sy) + v1 * sy;
}

// fbm_value_noise (:191-209)
GC_DEV double rd_fbm(double x, double y, int octaves, double gain, int64_t seed) {
  double value = 0.0, amplitude = 1.0, frequency = 1.0, max_amplitude = 0.0;
  for (int o = 0; o < octaves; ++o) {
    value += amplitude * rd_value_noise(x * frequency, y * frequency, seed);
    max_amplitude += amplitude;
    amplitude *= gain;
    frequency *= 2.0;
  }
  return value / (max_amplitude + 1e-12);
}

__global__ __launch_bounds__(kRdT) void k_fbm(int64_t n, const double* xy, int octaves, double gain, int64_t seed,
                                              double* out) {
  const int64_t i = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (i < n) out[i] = rd_fbm(xy[2 * i], xy[2 * i + 1], octaves, gain, seed);
}

// ------------------------------------------------------------------------------------------------
// BEV splat preparation
// ------------------------------------------------------------------------------------------------

struct BevCfg {
  double ox, oy, ppm, eps, gamma, logdet0, alpha_min, gain, s_f;
  int octaves;
  int64_t seed;
};

// per view P (6, row-major 2 x 3) then view_dir (3)
struct BevViews {
  double v[kRdMaxViews * 9];
};

__global__ __launch_bounds__(kRdT) void k_bev_prep(int64_t n, int n_views, gc_render_batch b, BevViews views, BevCfg c,
                                                   gc_bev_splats out) {
  const int64_t g = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (g >= n * n_views) return;
  const int v = (int)(g / n);
  const int64_t i = g - (int64_t)v * n;
  double P[6], vd[3], mu[3], S[9];
#pragma unroll
  for (int q = 0; q < 6; ++q) P[q] = views.v[9 * v + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    vd[q] = views.v[9 * v + 6 + q];
    mu[q] = b.mu_world[3 * i + q];
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) S[q] = b.Sigma_world[9 * i + q];
  // bev_pushforward.py:62-63: P mu and (P Sigma) P^T
  double mb[2], PS[6], Sb[4];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    mb[r] = P[3 * r] * mu[0] + P[3 * r + 1] * mu[1] + P[3 * r + 2] * mu[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) PS[3 * r + k] = P[3 * r] * S[k] + P[3 * r + 1] * S[3 + k] + P[3 * r + 2] * S[6 + k];
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 2; ++k) Sb[2 * r + k] = PS[3 * r] * P[3 * k] + PS[3 * r + 1] * P[3 * k + 1] + PS[3 * r + 2] * P[3 * k + 2];
  // the pixel map and the closed-form inverse of Sigma_px + eps I
  const double p2 = c.ppm * c.ppm;
  const double a = p2 * Sb[0] + c.eps, bb = p2 * Sb[1], cc = p2 * Sb[2], d = p2 * Sb[3] + c.eps;
  const double det = a * d - bb * cc;
  // opacity_from_logdet (rendering.py:243-244) of log det Sigma_bev
  const double logdet = log(Sb[0] * Sb[3] - Sb[1] * Sb[2]);
  const double raw = 1.0 / (1.0 + exp(-c.gamma * (c.logdet0 - logdet)));
  const double alpha = c.alpha_min + (1.0 - c.alpha_min) * raw;
  // vmf_shading_multi_lobe (:135-159): pi_b uniform, no intensity, mu_app = eta_b, kappa_app = |eta_b|
  const double s = rd_vmf_shading(b.eta, i, b.n_lobes, vd);
  // fbm at the splat's world (x, y) and the colour modulation (:333-340)
  const double f = rd_fbm(mu[0], mu[1], c.octaves, c.gain, c.seed);
  const double mod = (1.0 - c.s_f) + c.s_f * f;
  out.means_px[2 * g] = (mb[0] - c.ox) * c.ppm;
  out.means_px[2 * g + 1] = (mb[1] - c.oy) * c.ppm;
  out.Sigmas_inv[4 * g] = d / det;
  out.Sigmas_inv[4 * g + 1] = -bb / det;
  out.Sigmas_inv[4 * g + 2] = -cc / det;
  out.Sigmas_inv[4 * g + 3] = a / det;
  out.alphas[g] = alpha;
#pragma unroll
  for (int q = 0; q < 3; ++q) out.colors[3 * g + q] = b.color[3 * i + q] * s * mod;
  if (out.Sigmas_bev) {
#pragma unroll
    for (int q = 0; q < 4; ++q) out.Sigmas_bev[4 * g + q] = Sb[q];
  }
  if (v == 0) out.fbm[i] = f;
}

// ------------------------------------------------------------------------------------------------
// tile binning (rendering.py:252-289)
// ------------------------------------------------------------------------------------------------

// The binning key of splat i for segment seg (a (view, tile)): dist_sq to the tile centre, +inf where
// the four-sided bbox test rejects it (:283, the reference's strict inequalities).
GC_DEV double rd_bin_key(int64_t n, int64_t seg, const TileGrid& G, const double* means, const double* Sinv,
                         double eps, int64_t i) {
  int oxi, oyi;
  const int64_t v = rd_seg_tile(seg, G, oxi, oyi);
  const double ox = (double)oxi, oy = (double)oyi;
  const double* Si = Sinv + 4 * (v * n + i);
  // the smaller eigenvalue of the symmetric 2 x 2 (eigvalsh reads the lower triangle)
  const double lam = fmax(rd_eig_min2(Si[0], Si[2], Si[3]), eps);
  const double r = 2.0 / sqrt(lam);
  const double mx = means[2 * (v * n + i)], my = means[2 * (v * n + i) + 1];
  const double x_max = ox + (double)G.ts, y_max = oy + (double)G.ts;
  const bool rejected = mx + r < ox || mx - r > x_max || my + r < oy || my - r > y_max;
  const double dx = mx - (ox + 0.5 * (double)G.ts), dy = my - (oy + 0.5 * (double)G.ts);
  // two rounded squares and one rounded sum, as Python's dx ** 2 + dy ** 2 (no contraction)
  const double dist_sq = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
  return rejected ? HUGE_VAL : dist_sq;
}

// One workgroup per (view, tile), cap <= kRdMaxCap: the cap smallest survivors by (dist_sq, index)
// through the LDS selection of gc_renderdev.h (rd_select_smallest), the key being rd_bin_key.
struct BevKey {
  int64_t n, seg;
  TileGrid G;
  const double *means, *Sinv;
  double eps;
  GC_DEV double operator()(int64_t i) const { return rd_bin_key(n, seg, G, means, Sinv, eps, i); }
};

__global__ __launch_bounds__(kRdT) void k_bin_select(int64_t n, TileGrid G, const double* means, const double* Sinv,
                                                     double eps, int cap, int32_t* counts, int32_t* indices) {
  const int64_t seg = blockIdx.x;
  const BevKey key{n, seg, G, means, Sinv, eps};
  rd_select_smallest<false>(n, seg, key, cap, counts, nullptr, indices);
}

// The same through the library's sort, for a cap above kRdMaxCap (the one-tile entry only): the keys of
// the segments [seg0, seg0 + n_seg), the value is the splat index
__global__ __launch_bounds__(kRdT) void k_bin_keys(int64_t n, int64_t seg0, int64_t n_seg, TileGrid G,
                                                   const double* means, const double* Sinv, double eps, double* keys,
                                                   uint32_t* vals) {
  const int64_t g = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (g >= n_seg * n) return;
  const int64_t s = g / n, i = g - s * n;
  keys[g] = rd_bin_key(n, seg0 + s, G, means, Sinv, eps, i);
  vals[g] = (uint32_t)i;
}

// the first cap entries of every sorted segment: the index where the key is finite, else -1; the count
__global__ __launch_bounds__(kRdT) void k_bin_take(int64_t n, int64_t seg0, int64_t n_seg, int cap, const double* keys,
                                                   const uint32_t* vals, int32_t* counts, int32_t* indices) {
  const int64_t g = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (g >= n_seg * cap) return;
  const int64_t s = g / cap;
  const int c = (int)(g - s * cap);
  const bool in = c < n && keys[s * n + c] < HUGE_VAL;
  indices[(seg0 + s) * cap + c] = in ? (int32_t)vals[s * n + c] : -1;
  if (c == 0 && !in) counts[seg0 + s] = 0;
  if (in && (c == cap - 1 || c + 1 >= n || !(keys[s * n + c + 1] < HUGE_VAL))) counts[seg0 + s] = c + 1;
}

// ------------------------------------------------------------------------------------------------
// EWA raster (rendering.py:297-355)
// ------------------------------------------------------------------------------------------------

struct RasterArgs {
  int64_t n;          // splats per view
  TileGrid G;
  int H, W;           // image rows and columns per view
  const double *means, *Sinv, *alphas, *colors;
  const int32_t* indices;  // per segment `stride` entries; NULL: every splat in index order
  const int32_t* counts;   // per segment; NULL: n_list for every segment
  int64_t stride, n_list;
  double log_clip;
  double* images;
};

// One workgroup per (view, tile). The tile's list is staged kRdMaxCap records at a time in LDS; every
// lane reads the same record per step (a broadcast). Thread t owns pixels t, t + 256, t + 512, t + 768
// of the row-major tile and keeps their four sums in registers, in list order.
__global__ __launch_bounds__(kRdT) void k_raster(RasterArgs A) {
  __shared__ double rec[kRdMaxCap * kRdRec];
  const int64_t seg = blockIdx.x;
  const int ts = A.G.ts;
  int ox, oy;
  const int64_t v = rd_seg_tile(seg, A.G, ox, oy);
  const int64_t count = A.counts ? (int64_t)A.counts[seg] : A.n_list;
  constexpr int kPix = kRdMaxTile * kRdMaxTile / kRdT;
  double px[kPix], py[kPix], acc[kPix][3], wsum[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const int p = threadIdx.x + k * kRdT;
    px[k] = (double)(ox + p % ts) + 0.5;
    py[k] = (double)(oy + p / ts) + 0.5;
    acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    wsum[k] = 0.0;
  }
  for (int64_t base = 0; base < count; base += kRdMaxCap) {
    const int m = (int)((count - base) < kRdMaxCap ? (count - base) : kRdMaxCap);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const int64_t i = rd_list_index(A.indices ? (int64_t)A.indices[seg * A.stride + base + threadIdx.x] : base + threadIdx.x, A.n);
      const int64_t r = v * A.n + i;
      double* o = rec + kRdRec * threadIdx.x;
      o[0] = A.means[2 * r];
      o[1] = A.means[2 * r + 1];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[2 + q] = A.Sinv[4 * r + q];
      o[6] = A.alphas[r];
#pragma unroll
      for (int q = 0; q < 3; ++q) o[7 + q] = A.colors[3 * r + q];
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const double* o = rec + kRdRec * j;
      const double mx = o[0], my = o[1], s00 = o[2], s01 = o[3], s10 = o[4], s11 = o[5], al = o[6];
      const double c0 = o[7], c1 = o[8], c2 = o[9];
#pragma unroll
      for (int k = 0; k < kPix; ++k) {
        const double d0 = px[k] - mx, d1 = py[k] - my;
        const double q = rd_quad(d0, d1, s00, s01, s10, s11);
        const double arg = fmin(fmax(-0.5 * fmax(q, 0.0), -A.log_clip), 0.0);
        const double w = al * exp(arg);
        acc[k][0] += w * c0;
        acc[k][1] += w * c1;
        acc[k][2] += w * c2;
        wsum[k] += w;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const int p = threadIdx.x + k * kRdT;
    if (p >= ts * ts) continue;
    const double total = wsum[k] + 1e-12;  // :347
    const int64_t row = (oy - A.G.oy0) + p / ts, col = (ox - A.G.ox0) + p % ts;
    double* dst = A.images + ((v * A.H + row) * A.W + col) * 3;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double x = acc[k][q];
      if (total > 1e-12) x /= total;  // :353-354
      dst[q] = fmin(fmax(x, 0.0), 1.0);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

// splat_indices_for_tile for the segments of G (n_views * G.T of them, n splats each): counts (one per
// segment) and indices (cap per segment, -1 padded). n > 0, cap <= kRdMaxCap.
int rd_bin(gc_ctx* ctx, int64_t n, int64_t n_views, const TileGrid& G, const double* means, const double* Sinv,
           double eps, int cap, int32_t* counts, int32_t* indices) {
  hipLaunchKernelGGL(k_bin_select, dim3((unsigned)(n_views * G.T)), dim3(kRdT), 0, ctx->stream, n, G, means, Sinv, eps,
                     cap, counts, indices);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

// The same for one tile and any cap, through the library's stable sort (n < 2^31 keys in one segment);
// the count goes to a word of the scratch, returned in *count_word
int rd_bin_sorted(gc_ctx* ctx, int64_t n, const TileGrid& G, const double* means, const double* Sinv, double eps,
                  int cap, int32_t** count_word, int32_t* indices) {
  int32_t* count;
  double *keys_in, *keys;
  uint32_t *vals_in, *vals;
  void* tmp;
  if (int rc = carve_scratch(ctx, [&](Carver& c) {
        keys_in = c.take<double>((size_t)n);
        keys = c.take<double>((size_t)n);
        vals_in = c.take<uint32_t>((size_t)n);
        vals = c.take<uint32_t>((size_t)n);
        tmp = c.take<char>(sort_temp_bytes(1, n, true));
        count = c.take<int32_t>(1);
      }))
    return rc;
  *count_word = count;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_bin_keys, dim3(rd_blocks(n)), dim3(kRdT), 0, st, n, (int64_t)0, (int64_t)1, G, means, Sinv, eps,
                     keys_in, vals_in);
  GC_LAUNCH_CHECK(ctx);
  if (radix_sort_pairs(st, keys_in, keys, vals_in, vals, 1, n, false, tmp) != hipSuccess) {
    set_error(ctx, "the tile binning sort failed");
    return GC_ERR_RUNTIME;
  }
  hipLaunchKernelGGL(k_bin_take, dim3(rd_blocks(cap)), dim3(kRdT), 0, st, n, (int64_t)0, (int64_t)1, cap,
                     (const double*)keys, (const uint32_t*)vals, count, indices);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_renderable_batch_from_view(gc_ctx* ctx, const gc_map_view* view, double eps_lift, const gc_render_batch* out,
                                      int64_t* h_count) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, view && out && h_count, "NULL argument");
  GC_CHECK_ARG(ctx, view->n_tiles >= 0 && view->m_tile_view >= 0, "bad view shape");
  GC_CHECK_ARG(ctx, view->n_lobes >= 1 && view->n_lobes <= kMapMaxLobes && out->n_lobes == view->n_lobes,
               "n_lobes must be in [1, 8] and equal in the view and the batch");
  GC_CHECK_ARG(ctx, eps_lift == eps_lift, "NaN scalar argument");
  const int64_t V = (int64_t)view->n_tiles * view->m_tile_view;
  GC_CHECK_ARG(ctx, V < (int64_t)INT32_MAX, "view too large");
  *h_count = 0;
  if (V == 0) return GC_OK;
  GC_CHECK_ARG(ctx, view->valid_mask && view->positions && view->covariances && view->weights && view->primitive_ids &&
                        view->last_supported_scan_seq && view->etas && view->colors, "NULL view field");
  GC_CHECK_ARG(ctx, out->mu_world && out->Sigma_world && out->Lambda_world && out->eta && out->mass && out->color &&
                        out->primitive_ids && out->last_supported_scan_seq, "NULL batch field");
  double *k0, *k1;
  uint32_t *v0, *v1, *v2;
  int32_t* count;
  void* tmp;
  if (int rc = carve_scratch(ctx, [&](Carver& c) {
        k0 = c.take<double>((size_t)V);
        k1 = c.take<double>((size_t)V);
        v0 = c.take<uint32_t>((size_t)V);
        v1 = c.take<uint32_t>((size_t)V);
        v2 = c.take<uint32_t>((size_t)V);
        count = c.take<int32_t>(1);
        tmp = c.take<char>(sort_temp_bytes(1, V, true));
      }))
    return rc;
  hipStream_t st = ctx->stream;
  const unsigned nb = rd_blocks(V);
  GC_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_rb_keys_id, dim3(nb), dim3(kRdT), 0, st, V, (const uint8_t*)view->valid_mask,
                     (const int64_t*)view->primitive_ids, k0, v0, count);
  GC_LAUNCH_CHECK(ctx);
  if (radix_sort_pairs(st, k0, k1, v0, v1, 1, V, false, tmp) != hipSuccess) {
    set_error(ctx, "the primitive id sort failed");
    return GC_ERR_RUNTIME;
  }
  hipLaunchKernelGGL(k_rb_keys_seq, dim3(nb), dim3(kRdT), 0, st, V, (const uint8_t*)view->valid_mask,
                     (const int64_t*)view->last_supported_scan_seq, (const uint32_t*)v1, k0);
  GC_LAUNCH_CHECK(ctx);
  if (radix_sort_pairs(st, k0, k1, v1, v2, 1, V, true, tmp) != hipSuccess) {
    set_error(ctx, "the recency sort failed");
    return GC_ERR_RUNTIME;
  }
  hipLaunchKernelGGL(k_rb_gather, dim3(nb), dim3(kRdT), 0, st, V, *view, (const uint32_t*)v2, (const int32_t*)count,
                     eps_lift, *out);
  GC_LAUNCH_CHECK(ctx);
  int32_t h = 0;
  GC_HIP(ctx, hipMemcpyAsync(&h, count, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (int rc_w = wait_stream(ctx, st, "the renderable batch")) return rc_w;
  *h_count = h;
  return GC_OK;
}

int32_t gc_fbm_at_positions(gc_ctx* ctx, int64_t n, const double* d_xy, int32_t octaves, double gain, int64_t seed,
                            double* d_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, n >= 0 && n <= ((int64_t)1 << 28), "n must be in [0, 2^28]");
  GC_CHECK_ARG(ctx, octaves >= 0 && octaves <= 32, "octaves must be in [0, 32]");
  GC_CHECK_ARG(ctx, seed >= 0 && seed < ((int64_t)1 << 31), "seed must be in [0, 2^31)");
  GC_CHECK_ARG(ctx, gain == gain, "NaN scalar argument");
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, d_xy && d_out, "NULL buffer");
  hipLaunchKernelGGL(k_fbm, dim3(rd_blocks(n)), dim3(kRdT), 0, ctx->stream, n, d_xy, (int)octaves, gain, seed, d_out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_bev_splat_prep(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_views, const double* h_P,
                          const double* h_view_dirs, const gc_bev_cfg* cfg, const gc_bev_splats* out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, batch && h_P && h_view_dirs && cfg && out, "NULL argument");
  GC_CHECK_ARG(ctx, n >= 0 && n <= ((int64_t)1 << 24), "n must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, n_views >= 1 && n_views <= kRdMaxViews, "n_views must be in [1, 32]");
  GC_CHECK_ARG(ctx, batch->n_lobes >= 1 && batch->n_lobes <= kMapMaxLobes, "n_lobes must be in [1, 8]");
  GC_CHECK_ARG(ctx, cfg_all<11>(cfg, rd_finite), "the configuration must be finite");
  for (int q = 0; q < 6 * n_views; ++q) GC_CHECK_ARG(ctx, rd_finite(h_P[q]), "P must be finite");
  for (int q = 0; q < 3 * n_views; ++q) GC_CHECK_ARG(ctx, rd_finite(h_view_dirs[q]), "view_dirs must be finite");
  BevCfg c;
  c.ox = cfg->origin_x; c.oy = cfg->origin_y; c.ppm = cfg->px_per_m; c.eps = cfg->eps; c.gamma = cfg->opacity_gamma;
  c.logdet0 = cfg->logdet0; c.alpha_min = cfg->alpha_min; c.octaves = (int)cfg->fbm_octaves; c.gain = cfg->fbm_gain;
  c.seed = (int64_t)cfg->fbm_seed; c.s_f = cfg->fbm_modulate_scale;
  GC_CHECK_ARG(ctx, c.ppm > 0.0, "px_per_m must be > 0");
  GC_CHECK_ARG(ctx, cfg->fbm_octaves >= 0.0 && cfg->fbm_octaves <= 32.0 && cfg->fbm_octaves == floor(cfg->fbm_octaves),
               "fbm_octaves must be an integer in [0, 32]");
  GC_CHECK_ARG(ctx, cfg->fbm_seed >= 0.0 && cfg->fbm_seed < 2147483648.0 && cfg->fbm_seed == floor(cfg->fbm_seed),
               "fbm_seed must be an integer in [0, 2^31)");
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, batch->mu_world && batch->Sigma_world && batch->eta && batch->color, "NULL batch field");
  GC_CHECK_ARG(ctx, out->means_px && out->Sigmas_inv && out->alphas && out->colors && out->fbm, "NULL output field");
  BevViews views = {};
  for (int v = 0; v < n_views; ++v) {
    for (int q = 0; q < 6; ++q) views.v[9 * v + q] = h_P[6 * v + q];
    for (int q = 0; q < 3; ++q) views.v[9 * v + 6 + q] = h_view_dirs[3 * v + q];
  }
  hipLaunchKernelGGL(k_bev_prep, dim3(rd_blocks(n * n_views)), dim3(kRdT), 0, ctx->stream, n, (int)n_views, *batch,
                     views, c, *out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_render_ewa_tiles(gc_ctx* ctx, int32_t n_views, int64_t n, const gc_bev_splats* splats, int32_t H, int32_t W,
                            int32_t tile_size, int32_t cap, double log_clip, double eps, double* d_images,
                            int32_t* d_tile_counts, int32_t* d_tile_indices) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  TileGrid G;
  int64_t segs;
  if (int rc = rd_tile_grid(ctx, n_views, n, H, W, tile_size, kRdMaxTile, cap,
                            {"n_views must be in [1, 32]", "tile_size must be in [1, 32]",
                             "H and W must be multiples of tile_size in [1, 16384]",
                             "H and W must be multiples of tile_size in [1, 16384]", "n_views * tiles * n must be below 2^32"},
                            &G, &segs))
    return rc;
  GC_CHECK_ARG(ctx, log_clip == log_clip && eps == eps, "NaN scalar argument");
  GC_CHECK_ARG(ctx, d_images && d_tile_counts && d_tile_indices, "NULL output buffer");
  hipStream_t st = ctx->stream;
  if (n == 0) {
    GC_HIP(ctx, hipMemsetAsync(d_images, 0, sizeof(double) * 3 * (size_t)n_views * H * W, st));
    GC_HIP(ctx, hipMemsetAsync(d_tile_counts, 0, sizeof(int32_t) * (size_t)segs, st));
    GC_HIP(ctx, hipMemsetAsync(d_tile_indices, 0xFF, sizeof(int32_t) * (size_t)segs * cap, st));
    return GC_OK;
  }
  GC_CHECK_ARG(ctx, splats && splats->means_px && splats->Sigmas_inv && splats->alphas && splats->colors,
               "NULL splat field");
  if (int rc = rd_bin(ctx, n, n_views, G, splats->means_px, splats->Sigmas_inv, eps, cap, d_tile_counts, d_tile_indices))
    return rc;
  RasterArgs A;
  A.n = n; A.G = G; A.H = H; A.W = W;
  A.means = splats->means_px; A.Sinv = splats->Sigmas_inv; A.alphas = splats->alphas; A.colors = splats->colors;
  A.indices = d_tile_indices; A.counts = d_tile_counts; A.stride = cap; A.n_list = 0;
  A.log_clip = log_clip; A.images = d_images;
  hipLaunchKernelGGL(k_raster, dim3((unsigned)segs), dim3(kRdT), 0, st, A);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_splat_indices_for_tile(gc_ctx* ctx, int64_t n, const double* d_means, const double* d_Sigmas_inv,
                                  int32_t origin_y, int32_t origin_x, int32_t tile_size, int32_t cap, double eps,
                                  int32_t* d_indices, int32_t* h_count) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, tile_size >= 1 && tile_size <= kRdMaxTile, "tile_size must be in [1, 32]");
  GC_CHECK_ARG(ctx, n >= 0 && n < ((int64_t)1 << 31), "n must be in [0, 2^31)");
  GC_CHECK_ARG(ctx, cap >= 1 && cap <= (1 << 24), "cap must be in [1, 2^24]");
  GC_CHECK_ARG(ctx, abs(origin_y) <= (1 << 24) && abs(origin_x) <= (1 << 24), "tile origin outside [-2^24, 2^24]");
  GC_CHECK_ARG(ctx, eps == eps && h_count, "NaN or NULL argument");
  *h_count = 0;
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, d_means && d_Sigmas_inv && d_indices, "NULL buffer");
  TileGrid G;
  G.tiles_x = 1; G.T = 1; G.ts = tile_size; G.oy0 = origin_y; G.ox0 = origin_x;
  const int take = (int64_t)cap < n ? cap : (int)n;  // d_indices holds min(cap, n) entries
  int32_t* d_count;
  if (take <= kRdMaxCap) {
    if (int rc = carve_scratch(ctx, [&](Carver& c) { d_count = c.take<int32_t>(1); })) return rc;
    if (int rc = rd_bin(ctx, n, 1, G, d_means, d_Sigmas_inv, eps, take, d_count, d_indices)) return rc;
  } else if (int rc = rd_bin_sorted(ctx, n, G, d_means, d_Sigmas_inv, eps, take, &d_count, d_indices)) {
    return rc;
  }
  int32_t h = 0;
  GC_HIP(ctx, hipMemcpyAsync(&h, d_count, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (int rc_w = wait_stream(ctx, ctx->stream, "the tile binning")) return rc_w;
  *h_count = h;
  return GC_OK;
}

int32_t gc_render_tile_ewa(gc_ctx* ctx, int64_t n, const double* d_means, const double* d_Sigmas_inv,
                           const double* d_alphas, const double* d_colors, int32_t origin_y, int32_t origin_x,
                           int32_t tile_size, const int32_t* d_indices, int64_t n_idx, double log_clip,
                           double* d_image) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, tile_size >= 1 && tile_size <= kRdMaxTile, "tile_size must be in [1, 32]");
  GC_CHECK_ARG(ctx, n >= 0 && n < ((int64_t)1 << 31), "n must be in [0, 2^31)");
  GC_CHECK_ARG(ctx, n_idx >= -1 && n_idx < ((int64_t)1 << 31), "n_idx must be -1 (every splat) or in [0, 2^31)");
  GC_CHECK_ARG(ctx, n_idx <= 0 || d_indices, "NULL index buffer");
  GC_CHECK_ARG(ctx, abs(origin_y) <= (1 << 24) && abs(origin_x) <= (1 << 24), "tile origin outside [-2^24, 2^24]");
  GC_CHECK_ARG(ctx, log_clip == log_clip && d_image, "NaN or NULL argument");
  const int64_t n_list = n_idx < 0 ? n : n_idx;
  if (n == 0 || n_list == 0) {  // :324-327
    GC_HIP(ctx, hipMemsetAsync(d_image, 0, sizeof(double) * 3 * tile_size * tile_size, ctx->stream));
    return GC_OK;
  }
  GC_CHECK_ARG(ctx, d_means && d_Sigmas_inv && d_alphas && d_colors, "NULL splat buffer");
  RasterArgs A;
  A.n = n;
  A.G.tiles_x = 1; A.G.T = 1; A.G.ts = tile_size; A.G.oy0 = origin_y; A.G.ox0 = origin_x;
  A.H = tile_size; A.W = tile_size;
  A.means = d_means; A.Sinv = d_Sigmas_inv; A.alphas = d_alphas; A.colors = d_colors;
  A.indices = n_idx < 0 ? nullptr : d_indices; A.counts = nullptr; A.stride = 0; A.n_list = n_list;
  A.log_clip = log_clip; A.images = d_image;
  hipLaunchKernelGGL(k_raster, dim3(1), dim3(kRdT), 0, ctx->stream, A);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
