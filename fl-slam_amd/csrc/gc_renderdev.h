// gc_renderdev.h — what the BEV renderer (gc_render.hip) and the camera view (gc_camrender.hip) share
// (device code only): the limits of a tile, the tile grid, the 2 x 2 closed forms, the vMF shading and
// the per-(view, tile) LDS selection of the cap smallest survivors by (key, index).
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
