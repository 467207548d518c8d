// gc_renderdev.h — what the BEV renderer (gc_render.hip), the camera view (gc_camrender.hip) and the depth
// pose evidence (gc_depthev.hip) share. Host: the finiteness test, the blocks of a grid, the frame check that
// builds the tile grid; the camera view's checked configuration and packed views. Device: the (view, tile)
// decode, the clamped count and index, the 2 x 2 closed forms, the vMF shading, the LDS selection of a
// tile's cap smallest survivors; the camera view's projection of a primitive and its compositing step.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gc_internal.h"
#include "gc_math.h"

namespace gc {

constexpr int kRdT = 256;             // threads of every workgroup of the renderers
constexpr int kRdMaxTile = GC_RENDER_MAX_TILE;    // rendering.py:267, :320: tile_size is clamped to [1, 32]
constexpr int kRdMaxCap = GC_RENDER_MAX_CAP;      // splat records one raster step holds in LDS
constexpr int kRdMaxViews = GC_RENDER_MAX_VIEWS;  // the views travel by value as a kernel argument

struct TileGrid {
  int tiles_x, T;  // tiles per row and per view
  int ts;          // tile_size
  int oy0, ox0;    // origin of tile 0
};

// ---- host side
inline unsigned rd_blocks(int64_t threads) { return (unsigned)((threads + kRdT - 1) / kRdT); }

inline bool rd_finite(double x) { return fabs(x) <= 1e300; }

// the messages of a raster entry's frame checks: each entry keeps its own (one sentence may stand twice)
struct RdGridText { const char *views, *tile, *frame, *multiple, *segs; };

// The frame of n_views views of n splats cut into tile_size x tile_size tiles (tile_size <= max_tile) with
// lists of cap entries: every check, then the grid (origin 0) and the number of (view, tile) segments.
inline int rd_tile_grid(gc_ctx* ctx, int32_t n_views, int64_t n, int32_t H, int32_t W, int32_t tile_size, int max_tile,
                        int32_t cap, const RdGridText& text, TileGrid* G, int64_t* segs) {
  GC_CHECK_ARG(ctx, n_views >= 1 && n_views <= kRdMaxViews, text.views);
  GC_CHECK_ARG(ctx, tile_size >= 1 && tile_size <= max_tile, text.tile);
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && H <= 16384 && W <= 16384, text.frame);
  GC_CHECK_ARG(ctx, H % tile_size == 0 && W % tile_size == 0, text.multiple);
  GC_CHECK_ARG(ctx, cap >= 1 && cap <= kRdMaxCap, "cap must be in [1, 256]");
  GC_CHECK_ARG(ctx, n >= 0, "n must be >= 0");
  G->tiles_x = W / tile_size;
  G->T = G->tiles_x * (H / tile_size);
  G->ts = tile_size;
  G->oy0 = G->ox0 = 0;
  *segs = (int64_t)n_views * G->T;
  GC_CHECK_ARG(ctx, *segs < ((int64_t)1 << 31) && (n == 0 || *segs < ((int64_t)1 << 32) / n), text.segs);
  return GC_OK;
}

// the camera view's configuration, checked: its two entries and the depth evidence's two read it through this
struct CamCfg {
  double near, far, lowpass, radius_sigma, alpha_floor, alpha_max, alpha_skip, t_stop, bg[3], eps;
  int shade;
};

inline int cam_cfg(gc_ctx* ctx, const gc_camview_cfg* h, CamCfg* c) {
  GC_CHECK_ARG(ctx, h != nullptr, "NULL configuration");
  GC_CHECK_ARG(ctx, cfg_all<13>(h, rd_finite), "the configuration must be finite");
  c->near = h->near; c->far = h->far; c->lowpass = h->lowpass_px2; c->radius_sigma = h->radius_sigma;
  c->alpha_floor = h->alpha_floor; c->alpha_max = h->alpha_max; c->alpha_skip = h->alpha_skip; c->t_stop = h->t_stop;
  c->bg[0] = h->bg_r; c->bg[1] = h->bg_g; c->bg[2] = h->bg_b; c->shade = h->shade != 0.0;
  c->eps = h->eps;
  GC_CHECK_ARG(ctx, c->near > 0.0 && c->far > c->near, "near must be > 0 and far > near");
  GC_CHECK_ARG(ctx, c->alpha_max > 0.0 && c->alpha_max <= 1.0, "alpha_max must be in (0, 1]");
  return GC_OK;
}

// A packed view: R (9, row-major), t (3), fx fy cx cy, the camera centre -R^T t (3), the body position t_wb
// (3), the limits limx, limy of the clamped tangents (1.3 x the frame's half extent over the focal length).
// The views travel by value as a kernel argument, kCamViewsPerLaunch at a time (3072 B; with the batch, the
// configuration and the pointers k_cam_prep takes about 3.3 KB and k_ev_jvp 3.2 KB, below 4 KB).
constexpr int kCamView = 24, kCamViewsPerLaunch = 16;
enum { kCvR = 0, kCvT = 9, kCvFx = 12, kCvFy, kCvCx, kCvCy, kCvCentre = 16, kCvTwb = 19, kCvLimX = 22, kCvLimY = 23 };
struct CamViews { double v[kCamViewsPerLaunch * kCamView]; };
static_assert(kCamView % 2 == 0 && sizeof(CamViews) + 512 <= 4096, "the argument block stays below 4 KB");

// n_views views into out (kRdMaxViews * kCamView doubles), every argument checked; h_t_wb may be NULL (0)
inline int cam_pack_views(gc_ctx* ctx, int n_views, const double* h_T_cw, const double* h_intrinsics, const double* h_t_wb,
                          int32_t H, int32_t W, double* out) {
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "H and W must be in [1, 16384]");
  for (int v = 0; v < n_views; ++v) {
    const double* T = h_T_cw + 16 * v;
    const double* K = h_intrinsics + 4 * v;
    for (int q = 0; q < 16; ++q) GC_CHECK_ARG(ctx, rd_finite(T[q]), "T_cw must be finite");
    for (int q = 0; q < 4; ++q) GC_CHECK_ARG(ctx, rd_finite(K[q]), "the intrinsics must be finite");
    for (int q = 0; h_t_wb && q < 3; ++q) GC_CHECK_ARG(ctx, rd_finite(h_t_wb[3 * v + q]), "t_wb must be finite");
    GC_CHECK_ARG(ctx, K[0] > 0.0 && K[1] > 0.0, "fx and fy must be > 0");
    GC_CHECK_ARG(ctx, T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0, "the bottom row of T_cw must be (0, 0, 0, 1)");
    double* V = out + kCamView * v;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) V[3 * r + k] = T[4 * r + k];
      V[kCvT + r] = T[4 * r + 3];
    }
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) {
        const double g = V[r] * V[k] + V[3 + r] * V[3 + k] + V[6 + r] * V[6 + k] - (r == k ? 1.0 : 0.0);  // R^T R - I
        GC_CHECK_ARG(ctx, fabs(g) <= 1e-9, "the 3 x 3 block of T_cw must be a rotation");
      }
    for (int q = 0; q < 4; ++q) V[kCvFx + q] = K[q];
    for (int k = 0; k < 3; ++k) {
      V[kCvCentre + k] = -(V[k] * V[kCvT] + V[3 + k] * V[kCvT + 1] + V[6 + k] * V[kCvT + 2]);  // -R^T t
      V[kCvTwb + k] = h_t_wb ? h_t_wb[3 * v + k] : 0.0;
    }
    V[kCvLimX] = 1.3 * fmax(K[2], (double)W - K[2]) / K[0];
    V[kCvLimY] = 1.3 * fmax(K[3], (double)H - K[3]) / K[1];
  }
  return GC_OK;
}

// launch(v0, nv, views), a kernel launch, for every group of at most kCamViewsPerLaunch packed views, in order
template <typename Launch>
inline int cam_each_launch(gc_ctx* ctx, int n_views, const double* packed, Launch launch) {
  for (int v0 = 0; v0 < n_views; v0 += kCamViewsPerLaunch) {
    const int nv = n_views - v0 < kCamViewsPerLaunch ? n_views - v0 : kCamViewsPerLaunch;
    CamViews views = {};
    for (int q = 0; q < nv * kCamView; ++q) views.v[q] = packed[v0 * kCamView + q];
    launch(v0, nv, views);
    GC_LAUNCH_CHECK(ctx);
  }
  return GC_OK;
}

// ---- device side
// segment seg = (view v, tile t) of the grid: v, and the tile's pixel origin
GC_DEV int64_t rd_seg_tile(int64_t seg, const TileGrid& G, int& ox, int& oy) {
  const int64_t v = seg / G.T;
  const int t = (int)(seg - v * G.T);
  ox = G.ox0 + (t % G.tiles_x) * G.ts;
  oy = G.oy0 + (t / G.tiles_x) * G.ts;
  return v;
}

// a list's count as the raster trusts it: in [0, cap]
GC_DEV int rd_clamp_count(int m, int cap) { return m < 0 ? 0 : (m > cap ? cap : m); }

// entry `at` of the lists as a row the raster may read: in [0, n)
GC_DEV int64_t rd_list_index(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// (d @ Sigma_inv) @ d (rendering.py:85)
GC_DEV double rd_quad(double d0, double d1, double s00, double s01, double s10, double s11) {
  return (d0 * s00 + d1 * s10) * d0 + (d0 * s01 + d1 * s11) * d1;
}

// The eigenvalues of the symmetric 2 x 2 [[a, b], [b, d]] (eigvalsh reads the lower triangle):
// 0.5 (a + d) -+ sqrt((0.5 (a - d))^2 + b^2)
GC_DEV double rd_eig_min2(double a, double b, double d) {
  const double hd = 0.5 * (a - d);
  return 0.5 * (a + d) - sqrt(hd * hd + b * b);
}
GC_DEV double rd_eig_max2(double a, double b, double d) {
  const double hd = 0.5 * (a - d);
  return 0.5 * (a + d) + sqrt(hd * hd + b * b);
}

// vmf_shading_multi_lobe (rendering.py:135-159) of row i's L lobes for the view direction vd (not
// normalised): pi_b uniform, no intensity, mu_app = eta_b, kappa_app = |eta_b|
GC_DEV double rd_vmf_shading(const double* eta, int64_t i, int L, const double* vd) {
  const double nv = sqrt(vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2]) + 1e-12;
  const double v0 = vd[0] / nv, v1 = vd[1] / nv, v2 = vd[2] / nv;
  const double pi_b = 1.0 / (double)L;
  double s = 0.0, kappa_sum = 0.0;
  for (int l = 0; l < L; ++l) {
    const double e0 = eta[(i * L + l) * 3], e1 = eta[(i * L + l) * 3 + 1], e2 = eta[(i * L + l) * 3 + 2];
    const double kap = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    const double nm = kap + 1e-12;
    const double dot = (e0 / nm) * v0 + (e1 / nm) * v1 + (e2 / nm) * v2;
    s += pi_b * exp(kap * (dot - 1.0));
    kappa_sum += kap;
  }
  return s / (1.0 + kappa_sum / (double)L);
}

// The camera view of one primitive (mean mu, covariance S) through the packed view V: p = R mu + t, the
// tangents u = (x / z, y / z) and their clamped values times z, the Jacobian of the pinhole at the clamped
// tangents, M = J R and M S, the pixel mean. k_cam_prep renders with these and k_ev_jvp differentiates them.
struct CamProj {
  double p[3], ux, uy, tx, ty, J00, J02, J11, J12, M[6], MS[6], px, py;
};

GC_DEV void cam_project(const double* V, const double* mu, const double* S, CamProj& o) {
  const double* R = V + kCvR;
#pragma unroll
  for (int r = 0; r < 3; ++r) o.p[r] = R[3 * r] * mu[0] + R[3 * r + 1] * mu[1] + R[3 * r + 2] * mu[2] + V[kCvT + r];
  const double fx = V[kCvFx], fy = V[kCvFy], limx = V[kCvLimX], limy = V[kCvLimY];
  const double x = o.p[0], y = o.p[1], z = o.p[2];
  o.ux = x / z, o.uy = y / z;
  o.tx = fmin(fmax(o.ux, -limx), limx) * z, o.ty = fmin(fmax(o.uy, -limy), limy) * z;
  o.J00 = fx / z, o.J02 = -fx * o.tx / (z * z), o.J11 = fy / z, o.J12 = -fy * o.ty / (z * z);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.M[k] = o.J00 * R[k] + o.J02 * R[6 + k];
    o.M[3 + k] = o.J11 * R[3 + k] + o.J12 * R[6 + k];
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o.MS[3 * r + k] = o.M[3 * r] * S[k] + o.M[3 * r + 1] * S[3 + k] + o.M[3 * r + 2] * S[6 + k];
  o.px = fx * x / z + V[kCvCx];
  o.py = fy * y / z + V[kCvCy];
}

// One front-to-back compositing step. cam_step_alpha: the splat's opacity at a pixel, raw = al exp(-q / 2)
// and a = min(alpha_max, raw); a live pixel composites the splat where a >= alpha_skip (the comparison stays
// in the callers' branch: returned from here as a flag it cost k_ev_raster 3-4 %, its record reads no longer
// 16-byte). cam_step_through: the transmittance behind a composited splat; true where the pixel stops (the
// splat that crossed t_stop is composited).
GC_DEV void cam_step_alpha(double al, double q, double alpha_max, double& raw, double& a) {
  raw = al * exp(-0.5 * fmax(q, 0.0));
  a = fmin(alpha_max, raw);
}
GC_DEV bool cam_step_through(double& Tr, double a, double t_stop) {
  Tr *= 1.0 - a;
  return Tr < t_stop;
}

// The body of a selection kernel: one workgroup of kRdT threads per segment (a (view, tile)),
// cap <= kRdMaxCap. key(i) is splat i's key for this segment, +inf where the splat does not meet the
// tile. The splats are scanned 256 at a time in index order, the survivors (finite keys) appended to an
// LDS list in that order (ballot ranks, the waves' counts through LDS), and whenever the list holds
// more than cap entries it is cut back to its cap smallest by (key, index): every entry counts the
// entries below it, which is its place in the sorted list. The cap smallest of a prefix's cap smallest
// and the rest are the cap smallest of all, so the result is the first cap of the stable sort by key,
// whatever the chunking. With kSurvivors the number of survivors before any cut goes to survivors[seg].
constexpr int kBinBuf = kRdMaxCap + kRdT;

template <bool kSurvivors, typename Key>
GC_DEV void rd_select_smallest(int64_t n, int64_t seg, const Key& key, int cap, int32_t* counts, int32_t* survivors,
                               int32_t* indices) {
  __shared__ double cd[kBinBuf], td[kRdMaxCap];
  __shared__ int32_t ci[kBinBuf], ti[kRdMaxCap];
  __shared__ int wcnt[kRdT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int count = 0;  // the same in every thread
  int seen = 0;   // the survivors so far, before any cut
  // the list cut back to min(count, cap) entries, sorted
  auto cut = [&]() {
    const int keep = count < cap ? count : cap;
    for (int e = tid; e < count; e += kRdT) {
      const double de = cd[e];
      const int32_t ie = ci[e];
      int r = 0;
      for (int j = 0; j < count; ++j) {
        const double dj = cd[j];
        r += (dj < de || (dj == de && ci[j] < ie)) ? 1 : 0;
      }
      if (r < keep) {
        td[r] = de;
        ti[r] = ie;
      }
    }
    __syncthreads();
    for (int e = tid; e < keep; e += kRdT) {
      cd[e] = td[e];
      ci[e] = ti[e];
    }
    __syncthreads();
    count = keep;
  };
  for (int64_t base = 0; base < n; base += kRdT) {
    const int64_t i = base + tid;
    double d = HUGE_VAL;
    if (i < n) d = key(i);
    const bool in = d < HUGE_VAL;
    const unsigned long long m = __ballot(in);
    if (lane == 0) wcnt[w] = (int)__popcll(m);
    __syncthreads();
    int pre = 0, total = 0;
#pragma unroll
    for (int u = 0; u < kRdT / 64; ++u) {
      pre += u < w ? wcnt[u] : 0;
      total += wcnt[u];
    }
    if (in) {
      const int at = count + pre + (int)__popcll(m & ((1ull << lane) - 1ull));
      cd[at] = d;
      ci[at] = (int32_t)i;
    }
    __syncthreads();
    count += total;
    if (kSurvivors) seen += total;
    if (count > cap) cut();
  }
  cut();
  for (int c = tid; c < cap; c += kRdT) indices[seg * cap + c] = c < count ? ci[c] : -1;
  if (tid == 0) {
    counts[seg] = count;
    if (kSurvivors) survivors[seg] = seen;
  }
}

}  // namespace gc
