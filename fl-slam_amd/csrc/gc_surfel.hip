// gc_surfel.hip — LiDAR surfel extraction on the device: the MeasurementBatch the OT association and
// VisualPoseEvidence consume, from the deskewed points of one scan.
//
//  extract_lidar_surfels / _extract_surfels_mahex3d_jax_jit   backend/operators/lidar_surfel_extraction.py:219-431
//  _fit_one_cell (weighted plane fit, Wishart regularisation)  :84-163
//  hex_cell_3d_batch / bin_points_3d (MA-hex hash grid)        common/ma_hex_web.py:221-303
//  measurement_batch_add_lidar_surfels (info form, vMF lobe)   backend/structures/measurement_batch.py:262-347
//
// Six kernels, f64, no floating-point atomics and no slot claiming: every sum and every slot has a
// fixed order, so a batch is bitwise the same from run to run.
//
//  k_sf_center   the masked weighted sums Σ p w, Σ w: per-workgroup partials (lane-local in index order,
//                xor butterfly, waves in wave order); the grid depends on N alone.
//  k_sf_keys     every workgroup adds the partials in the same fixed order (sf_center), then for its
//                tile of 1,024 points: the hash cell of each unmasked centred point and the point's rank
//                among the earlier points of the tile in the same cell. Four rounds of 256 points; in a
//                round a point's rank inside its wave comes from 14 ballots (the lanes that agree on
//                every key bit), the waves then take their turn in wave order against a per-cell running
//                count in LDS. The final running counts are the tile's histogram: hist[tile][cell].
//  k_sf_scan     per cell: the exclusive prefix of its counts over the tiles, in place, and the total.
//  k_sf_scatter  per point: slot = prefix[tile][cell] + rank; slots below max_occupants go to
//                bucket[cell][slot]. This is a stable counting sort cut off at max_occupants: a cell
//                keeps its first points in ascending point index, as the reference's stable argsort does.
//  k_sf_fit      eight lanes per cell: the weighted plane fit over the occupants (lane-local in slot
//                order, then an xor butterfly), the regularised covariance, and the cell's finished
//                batch row as a record.
//  k_sf_write    one lane per cell: the prefix sum of the n_cells validity flags (ascending cell id;
//                each workgroup counts the flags before its range, then scans its own), then rows
//                n_feat + j, j < n_valid = min(valid cells, n_surfel), and n_valid itself.
//
// Masked points (a coordinate at or beyond 0.1 x the non-finite sentinel, or NaN) take no part in
// any sum: the reference multiplies them by a zero weight, which is the same for finite values.
#include <hip/hip_runtime.h>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"

namespace gc {
namespace {

constexpr int kSfT = 256;                    // threads per workgroup (centre, keys, scan, scatter)
constexpr int kSfMaxGrid = 256;               // centre workgroups
constexpr int kSfTile = 1024;                 // points per ranking tile
constexpr int kSfRounds = kSfTile / kSfT;
constexpr int kSfKeyBits = 14;                // cell keys are below 2^14
constexpr int kSfMaxCells = GC_SURFEL_MAX_CELLS;
constexpr int kSfMaxOcc = GC_SURFEL_MAX_OCCUPANTS;  // bucket slots per cell
constexpr int64_t kSfMaxPoints = GC_SURFEL_MAX_POINTS;
constexpr int kSfFitT = 256, kSfFitLanes = 8;  // fit: eight lanes per cell, 32 cells per workgroup
constexpr int kSfWriteT = 256;
constexpr int kSfRec = 18;                    // Λ_row (9) | θ (3) | κ n (3) | w | t | grey
constexpr double kSfSentinel = 1e6;           // GC_NONFINITE_SENTINEL (common/constants.py)
constexpr double kSfEps = 1e-12;              // _fit_one_cell's eps default (:99), _normalize's eps (:69)

struct SfCfg {
  int n_surfel, n_feat, n1, n2, nz, max_occ, min_points, n_lobes;
  double h, sensor_var, nu, psi, kappa_scale, kappa_min, kappa_max, eig_min, eps_lift;
};

GC_DEV bool sf_unmasked(double x, double y, double z) {
  const double lim = 0.1 * kSfSentinel;
  return fabs(x) < lim && fabs(y) < lim && fabs(z) < lim;  // false for NaN
}

__global__ void __launch_bounds__(kSfT) k_sf_center(int64_t N, const double* __restrict__ pts,
                                                    const double* __restrict__ w, double* __restrict__ partial) {
  __shared__ double red[(kSfT / 64) * 4];
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kSfT + threadIdx.x; i < N; i += (int64_t)gridDim.x * kSfT) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2], wi = w[i];
    if (sf_unmasked(x, y, z)) {
      a[0] += x * wi;
      a[1] += y * wi;
      a[2] += z * wi;
      a[3] += wi;
    }
  }
  block_sum_stage<4>(a, red);
  if (threadIdx.x < 4)
    partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = block_sum_total<4, kSfT / 64>(red, threadIdx.x);
}

// center = Σ p w / (Σ w + eig_min) (lidar_surfel_extraction.py:265-266) from the G partials, added by the
// 256 threads of a workgroup in an order that depends on G alone (sum_partials: 4 columns, 64 chains).
// cen (LDS, 3) on return.
GC_DEV void sf_center(int G, const double* __restrict__ partial, double eig_min, double* stage /* kSfT */,
                      double* cen /* 4 */) {
  sum_partials<4, kSfT>(G, partial, 4, stage, cen);
  const double den = cen[3] + eig_min;
  __syncthreads();
  if (threadIdx.x < 3) cen[threadIdx.x] = cen[threadIdx.x] / den;
  __syncthreads();
}

// floor-mod of floor(s / h) by n (ma_hex_web.py:237-239, :264): non-negative for negative cells
GC_DEV int sf_wrap(double s, double h, int n) {
  const long long c = (long long)floor(s / h);
  const long long m = c % n;
  return (int)(m < 0 ? m + n : m);
}

__global__ void __launch_bounds__(kSfT) k_sf_keys(int64_t N, const double* __restrict__ pts, int G,
                                                  const double* __restrict__ partial, SfCfg cfg, int n_cells,
                                                  double* __restrict__ center_out, int32_t* __restrict__ keys,
                                                  int32_t* __restrict__ trank, uint32_t* __restrict__ hist) {
  __shared__ unsigned short run[kSfMaxCells];  // a tile holds 1,024 points: the counts fit 16 bits
  __shared__ double stage[kSfT];
  __shared__ double cen[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  sf_center(G, partial, cfg.eig_min, stage, cen);
  if (blockIdx.x == 0 && t < 3) center_out[t] = cen[t];
  for (int c = t; c < n_cells; c += kSfT) run[c] = 0;
  __syncthreads();
  const double h = fmax(cfg.h, 1e-12), k32 = 0.8660254037844386;  // √3 / 2
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = 0; r < kSfRounds; ++r) {
    const int64_t i = (int64_t)blockIdx.x * kSfTile + r * kSfT + t;
    bool valid = false;
    int key = 0;
    if (i < N) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      if (sf_unmasked(x, y, z)) {
        valid = true;
        const double xc = x - cen[0], yc = y - cen[1], zc = z - cen[2];
        const int c1 = sf_wrap(xc, h, cfg.n1), c2 = sf_wrap(xc * 0.5 + yc * k32, h, cfg.n2),
                  cz = sf_wrap(zc, h, cfg.nz);
        key = c1 * (cfg.n2 * cfg.nz) + c2 * cfg.nz + cz;
      }
    }
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < kSfKeyBits; ++b) {
      const unsigned long long m = __ballot(valid && ((key >> b) & 1));
      peers &= ((key >> b) & 1) ? m : ~m;
    }
    const int rank = __popcll(peers & lt), cnt = __popcll(peers);
    int mine = 0;
    for (int u = 0; u < kSfT / 64; ++u) {  // the waves in wave order: earlier points first
      if (u == wv && valid) {
        const int r0 = run[key];
        mine = r0 + rank;
        if (rank == cnt - 1) run[key] = (unsigned short)(r0 + cnt);  // the group's last lane, after every read
      }
      __syncthreads();
    }
    if (i < N) {
      keys[i] = valid ? key : -1;
      trank[i] = mine;
    }
  }
  for (int c = t; c < n_cells; c += kSfT) hist[(int64_t)blockIdx.x * n_cells + c] = run[c];
}

__global__ void __launch_bounds__(kSfT) k_sf_scan(int n_cells, int n_tiles, uint32_t* __restrict__ hist,
                                                  int32_t* __restrict__ count) {
  const int c = blockIdx.x * kSfT + threadIdx.x;
  if (c >= n_cells) return;
  uint32_t runc = 0;
  for (int b0 = 0; b0 < n_tiles; b0 += 8) {  // eight loads in flight, then their prefixes
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = b0 + u < n_tiles ? hist[(int64_t)(b0 + u) * n_cells + c] : 0u;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (b0 + u < n_tiles) hist[(int64_t)(b0 + u) * n_cells + c] = runc;
      runc += v[u];
    }
  }
  count[c] = (int32_t)runc;
}

__global__ void __launch_bounds__(kSfT) k_sf_scatter(int64_t N, const int32_t* __restrict__ keys,
                                                     const int32_t* __restrict__ trank,
                                                     const uint32_t* __restrict__ hist, int n_cells, int max_occ,
                                                     int32_t* __restrict__ bucket) {
  const int64_t i = (int64_t)blockIdx.x * kSfT + threadIdx.x;
  if (i >= N) return;
  const int key = keys[i];
  if (key < 0 || key >= n_cells) return;
  const int64_t slot = (int64_t)hist[(i / kSfTile) * n_cells + key] + trank[i];
  if (slot < max_occ) bucket[(int64_t)key * max_occ + slot] = (int32_t)i;
}

GC_DEV void sf_normalize(double* v) {  // _normalize (:69-70)
  const double n = norm3(v) + kSfEps;
  v[0] /= n; v[1] /= n; v[2] /= n;
}

GC_DEV void sf_sym_lift(double* A, double lift) {  // 0.5 (A + Aᵀ) + lift I
  const double a01 = 0.5 * (A[1] + A[3]), a02 = 0.5 * (A[2] + A[6]), a12 = 0.5 * (A[5] + A[7]);
  A[1] = a01; A[3] = a01; A[2] = a02; A[6] = a02; A[5] = a12; A[7] = a12;
  A[0] += lift; A[4] += lift; A[8] += lift;
}

__global__ void __launch_bounds__(kSfFitT) k_sf_fit(int64_t N, const double* __restrict__ pts,
                                                    const double* __restrict__ ts, const double* __restrict__ w,
                                                    const double* __restrict__ center, const int32_t* __restrict__ count,
                                                    const int32_t* __restrict__ bucket, SfCfg cfg, int n_cells,
                                                    double* __restrict__ rec, int32_t* __restrict__ flag) {
  // kSfFitLanes lanes per cell: lane `sub` adds the occupants sub, sub + 8, ... in slot order, then an
  // xor butterfly inside the group gives every lane the same total; the lanes of a group leave together
  const int sub = threadIdx.x & (kSfFitLanes - 1);
  const int c = (int)(((int64_t)blockIdx.x * kSfFitT + threadIdx.x) / kSfFitLanes);
  if (c >= n_cells) return;
  const int cnt = min(count[c], cfg.max_occ);  // ma_hex_web.py:302
  if (cnt <= 0) {  // an empty cell: w_surfel = 0, never valid
    if (sub == 0) flag[c] = 0;
    return;
  }
  const double cen[3] = {center[0], center[1], center[2]};
  const int32_t* occ = bucket + (int64_t)c * cfg.max_occ;
  // :121-122, :159-160 — Σ w, Σ w p, Σ t over the occupants
  double a1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // Σ w | Σ w p (3) | Σ t
  for (int s = sub; s < cnt; s += kSfFitLanes) {
    int64_t i = occ[s];
    i = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    const double wi = w[i];
    a1[0] += wi;
    a1[1] += (pts[3 * i] - cen[0]) * wi;
    a1[2] += (pts[3 * i + 1] - cen[1]) * wi;
    a1[3] += (pts[3 * i + 2] - cen[2]) * wi;
    a1[4] += ts[i];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) a1[q] = group_sum_xor<kSfFitLanes>(a1[q]);
  const double ws = a1[0], st = a1[4];
  const double w_sum = ws + kSfEps;
  const double mu[3] = {a1[1] / w_sum, a1[2] / w_sum, a1[3] / w_sum};
  // :124-126 — Σ w d dᵀ / w_sum about the centroid
  double a2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // xx xy xz yy yz zz
  for (int s = sub; s < cnt; s += kSfFitLanes) {
    int64_t i = occ[s];
    i = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    const double wi = w[i];
    const double dx = (pts[3 * i] - cen[0]) - mu[0], dy = (pts[3 * i + 1] - cen[1]) - mu[1],
                 dz = (pts[3 * i + 2] - cen[2]) - mu[2];
    a2[0] += wi * dx * dx; a2[1] += wi * dx * dy; a2[2] += wi * dx * dz;
    a2[3] += wi * dy * dy; a2[4] += wi * dy * dz; a2[5] += wi * dz * dz;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) a2[q] = group_sum_xor<kSfFitLanes>(a2[q]);
  const double cxx = a2[0], cxy = a2[1], cxz = a2[2], cyy = a2[3], cyz = a2[4], czz = a2[5];
  const double Cr[9] = {cxx / w_sum, cxy / w_sum, cxz / w_sum, cxy / w_sum, cyy / w_sum,
                        cyz / w_sum, cxz / w_sum, cyz / w_sum, czz / w_sum};
  double cov[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) cov[q] = Cr[q] + ((q % 4 == 0) ? cfg.eig_min : 0.0);
  // :128-131 — the eigenvector of the smallest eigenvalue, n_z >= 0, normalised
  double ev[3], V[9];
  eigh3(cov, ev, V);
  double l0 = ev[0], n[3] = {V[0], V[3], V[6]};
  if (ev[1] < l0) { l0 = ev[1]; n[0] = V[1]; n[1] = V[4]; n[2] = V[7]; }
  if (ev[2] < l0) { l0 = ev[2]; n[0] = V[2]; n[1] = V[5]; n[2] = V[8]; }
  if (n[2] < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
  sf_normalize(n);
  // :72-81 — the basis takes the normal normalised once more
  double n2[3] = {n[0], n[1], n[2]};
  sf_normalize(n2);
  double e1[3], e2[3];
  if (fabs(n2[2]) < 0.9) { e1[0] = -n2[1]; e1[1] = n2[0]; e1[2] = 0.0; }
  else { e1[0] = -n2[2]; e1[1] = 0.0; e1[2] = n2[0]; }
  sf_normalize(e1);
  cross3(n2, e1, e2);
  sf_normalize(e2);
  // :134-140 — Σ w (d·e)² / w_sum = eᵀ C e with the unlifted C
  double Ce[3];
  mat3_vec(Cr, e1, Ce);
  const double var_e1 = dot3(e1, Ce) + cfg.sensor_var;
  mat3_vec(Cr, e2, Ce);
  const double var_e2 = dot3(e2, Ce) + cfg.sensor_var;
  const double sig_perp = fmax(l0, cfg.eig_min);
  const double var_perp = sig_perp + cfg.sensor_var;
  const double d1 = fmax(var_e1, cfg.eig_min), d2 = fmax(var_e2, cfg.eig_min), d3 = fmax(var_perp, cfg.eig_min);
  // :142-154 — Σ = V D Vᵀ, Wishart regularisation in precision space
  double S[9], Lm[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) S[3 * a + b] = d1 * e1[a] * e1[b] + d2 * e2[a] * e2[b] + d3 * n[a] * n[b];
  sf_sym_lift(S, cfg.eig_min);
  S[0] += cfg.eig_min; S[4] += cfg.eig_min; S[8] += cfg.eig_min;  // inv(Σ + eig_min I)
  inv3(S, Lm);
  sf_sym_lift(Lm, 0.0);
  const double wish = cfg.nu / fmax(cfg.psi, kSfEps);
  Lm[0] += wish; Lm[4] += wish; Lm[8] += wish;
  sf_sym_lift(Lm, cfg.eig_min);
  inv3(Lm, S);
  sf_sym_lift(S, cfg.eig_min);  // Σ_reg
  // :156-162
  const double kappa = clampd(cfg.kappa_scale / sqrt(fmax(sig_perp, cfg.eig_min)), cfg.kappa_min, cfg.kappa_max);
  const bool ok = cnt >= cfg.min_points && ws > 0.0;
  if (sub != 0) return;  // every lane of the group holds the same values: one writes
  flag[c] = ok ? 1 : 0;
  if (!ok) return;
  // measurement_batch.py:299-312 — the info form of the row, the vMF lobe and the grey
  S[0] += cfg.eps_lift; S[4] += cfg.eps_lift; S[8] += cfg.eps_lift;
  inv3(S, Lm);
  const double pos[3] = {mu[0] + cen[0], mu[1] + cen[1], mu[2] + cen[2]};
  double th[3];
  mat3_vec(Lm, pos, th);
  double* r = rec + (int64_t)c * kSfRec;
#pragma unroll
  for (int q = 0; q < 9; ++q) r[q] = Lm[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    r[9 + q] = th[q];
    r[12 + q] = kappa * n[q];
  }
  r[15] = ws;
  r[16] = st / w_sum;
  r[17] = 0.25 + 0.5 * (clampd(n[2], -1.0, 1.0) + 1.0) / 2.0;
}

__global__ void __launch_bounds__(kSfWriteT) k_sf_write(int n_cells, const int32_t* __restrict__ flag,
                                                        const double* __restrict__ rec, SfCfg cfg,
                                                        double* __restrict__ Lam, double* __restrict__ tht,
                                                        double* __restrict__ eta, double* __restrict__ wts,
                                                        int32_t* __restrict__ src, int32_t* __restrict__ sidx,
                                                        uint8_t* __restrict__ valid, double* __restrict__ tst,
                                                        double* __restrict__ col, int32_t* __restrict__ slot_cells,
                                                        int32_t* __restrict__ n_valid_out) {
  // One cell per thread. A workgroup first counts the valid cells before its range (integers: any
  // order gives the same count), then scans its own 256 flags; the last workgroup knows the total.
  __shared__ int wsum[kSfWriteT / 64], wtot[kSfWriteT / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int first = blockIdx.x * kSfWriteT, c = first + t;
  int before = 0;
  for (int j = t; j < first; j += kSfWriteT) before += flag[j];
  before = group_sum_xor<64>(before);
  const int f = c < n_cells ? flag[c] : 0;
  int x = f;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 0) wsum[wv] = before;
  if (lane == 63) wtot[wv] = x;
  __syncthreads();
  int base = 0, pre = 0, mine = 0;
  for (int u = 0; u < kSfWriteT / 64; ++u) {
    base += wsum[u];
    pre += u < wv ? wtot[u] : 0;
    mine += wtot[u];
  }
  const int slot = base + pre + x - f;  // valid cells before this one, in ascending cell id
  if (f && slot < cfg.n_surfel) {
    const int64_t row = (int64_t)cfg.n_feat + slot;
    const double* r = rec + (int64_t)c * kSfRec;
    double v[kSfRec];
#pragma unroll
    for (int q = 0; q < kSfRec; ++q) v[q] = r[q];
#pragma unroll
    for (int q = 0; q < 9; ++q) Lam[9 * row + q] = v[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      tht[3 * row + q] = v[9 + q];
      eta[(row * cfg.n_lobes) * 3 + q] = v[12 + q];
      col[3 * row + q] = v[17];
    }
    for (int q = 3; q < 3 * cfg.n_lobes; ++q) eta[(row * cfg.n_lobes) * 3 + q] = 0.0;
    wts[row] = v[15];
    tst[row] = v[16];
    src[row] = 1;
    sidx[row] = slot;
    valid[row] = 1;
    if (slot_cells) slot_cells[slot] = c;
  }
  if (blockIdx.x == gridDim.x - 1) {
    const int n_valid = min(base + mine, cfg.n_surfel);
    if (slot_cells)
      for (int j = n_valid + t; j < cfg.n_surfel; j += kSfWriteT) slot_cells[j] = -1;
    if (t == 0) n_valid_out[0] = n_valid;
  }
}

static_assert(kSfMaxCells == 1 << kSfKeyBits, "k_sf_keys walks kSfKeyBits bits of a cell key");

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_extract_lidar_surfels(gc_ctx* ctx, int64_t N, const double* d_points, const double* d_timestamps,
                                 const double* d_weights, const gc_surfel_cfg* h, double* d_Lambdas, double* d_thetas,
                                 double* d_etas, double* d_weights_out, int32_t* d_sources,
                                 int32_t* d_source_indices, uint8_t* d_valid_mask, double* d_timestamps_out,
                                 double* d_colors, int32_t* d_slot_cells, int32_t* h_n_valid) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, h && h_n_valid, "NULL argument");
  GC_CHECK_ARG(ctx, N >= 0 && N <= kSfMaxPoints, "N must be in [0, 4194304]");
  GC_CHECK_ARG(ctx, N == 0 || (d_points && d_timestamps && d_weights), "NULL point buffer");
  GC_CHECK_ARG(ctx, d_Lambdas && d_thetas && d_etas && d_weights_out && d_sources && d_source_indices &&
                        d_valid_mask && d_timestamps_out && d_colors, "NULL batch buffer");
  GC_CHECK_ARG(ctx, gc::cfg_all<17>(h, [](double v) { return v == v; }), "NaN in the configuration");
  const auto as_int = [](double v, double lo, double hi, int* out) {
    if (!(v >= lo && v <= hi) || v != floor(v)) return false;
    *out = (int)v;
    return true;
  };
  SfCfg cfg;
  GC_CHECK_ARG(ctx, as_int(h->n_surfel, 1, 1 << 24, &cfg.n_surfel), "n_surfel must be in [1, 2^24]");
  GC_CHECK_ARG(ctx, as_int(h->n_feat, 0, 1 << 24, &cfg.n_feat), "n_feat must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, h->voxel_size_m > 0.0 && 2e5 / h->voxel_size_m < 2147483648.0,
               "voxel_size_m must be > 0 and 2e5 / voxel_size_m < 2^31");
  GC_CHECK_ARG(ctx, as_int(h->hex3d_num_cells_1, 1, kSfMaxCells, &cfg.n1) &&
                        as_int(h->hex3d_num_cells_2, 1, kSfMaxCells, &cfg.n2) &&
                        as_int(h->hex3d_num_cells_z, 1, kSfMaxCells, &cfg.nz), "grid sizes must be in [1, 16384]");
  const int64_t n_cells64 = (int64_t)cfg.n1 * cfg.n2 * cfg.nz;
  GC_CHECK_ARG(ctx, n_cells64 <= kSfMaxCells, "the grid must hold at most 16384 cells");
  GC_CHECK_ARG(ctx, as_int(h->hex3d_max_occupants, 1, kSfMaxOcc, &cfg.max_occ), "max_occupants must be in [1, 1024]");
  GC_CHECK_ARG(ctx, as_int(h->min_points_per_voxel, -(1 << 24), 1 << 24, &cfg.min_points), "min_points_per_voxel out of range");
  GC_CHECK_ARG(ctx, as_int(h->n_lobes, 1, 8, &cfg.n_lobes), "n_lobes must be in [1, 8]");
  cfg.h = h->voxel_size_m; cfg.sensor_var = h->sensor_noise_var_per_axis; cfg.nu = h->wishart_nu;
  cfg.psi = h->wishart_psi_scale; cfg.kappa_scale = h->kappa_main_scale; cfg.kappa_min = h->kappa_min;
  cfg.kappa_max = h->kappa_max; cfg.eig_min = h->eig_min; cfg.eps_lift = h->eps_lift;
  const int n_cells = (int)n_cells64;
  const int64_t blocks = (N + kSfT - 1) / kSfT;
  const int G = (int)(blocks < 1 ? 1 : (blocks > kSfMaxGrid ? kSfMaxGrid : blocks));
  const int64_t tiles64 = (N + kSfTile - 1) / kSfTile;
  const int n_tiles = (int)(tiles64 < 1 ? 1 : tiles64);
  const size_t npt = (size_t)(N > 0 ? N : 1);
  double *partial, *center, *rec;
  int32_t *keys, *trank, *count, *flag, *bucket, *d_nv;
  uint32_t* hist;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        partial = c.take<double>(4 * (size_t)G);
        center = c.take<double>(4);
        keys = c.take<int32_t>(npt);
        trank = c.take<int32_t>(npt);
        hist = c.take<uint32_t>((size_t)n_tiles * n_cells);
        count = c.take<int32_t>(n_cells);
        flag = c.take<int32_t>(n_cells);
        bucket = c.take<int32_t>((size_t)n_cells * cfg.max_occ);
        rec = c.take<double>(kSfRec * (size_t)n_cells);
        d_nv = c.take<int32_t>(1);
      }))
    return rc;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_sf_center, dim3((unsigned)G), dim3(kSfT), 0, st, N, d_points, d_weights, partial);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_sf_keys, dim3((unsigned)n_tiles), dim3(kSfT), 0, st, N, d_points, G, (const double*)partial, cfg,
                     n_cells, center, keys, trank, hist);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_sf_scan, dim3((unsigned)((n_cells + kSfT - 1) / kSfT)), dim3(kSfT), 0, st, n_cells, n_tiles, hist,
                     count);
  GC_LAUNCH_CHECK(ctx);
  if (N > 0) {
    hipLaunchKernelGGL(k_sf_scatter, dim3((unsigned)blocks), dim3(kSfT), 0, st, N, (const int32_t*)keys,
                       (const int32_t*)trank, (const uint32_t*)hist, n_cells, cfg.max_occ, bucket);
    GC_LAUNCH_CHECK(ctx);
  }
  const unsigned g_fit = (unsigned)(((int64_t)n_cells * kSfFitLanes + kSfFitT - 1) / kSfFitT),
                 g_write = (unsigned)((n_cells + kSfWriteT - 1) / kSfWriteT);
  hipLaunchKernelGGL(k_sf_fit, dim3(g_fit), dim3(kSfFitT), 0, st, N, d_points, d_timestamps, d_weights,
                     (const double*)center, (const int32_t*)count, (const int32_t*)bucket, cfg, n_cells, rec, flag);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_sf_write, dim3(g_write), dim3(kSfWriteT), 0, st, n_cells, (const int32_t*)flag,
                     (const double*)rec, cfg, d_Lambdas, d_thetas, d_etas, d_weights_out, d_sources, d_source_indices,
                     d_valid_mask, d_timestamps_out, d_colors, d_slot_cells, d_nv);
  GC_LAUNCH_CHECK(ctx);
  int32_t nv = 0;
  GC_HIP(ctx, hipMemcpyAsync(&nv, d_nv, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (int rc_w = gc::wait_stream(ctx, st, "the surfel count")) return rc_w;
  *h_n_valid = nv;
  return GC_OK;
}

}  // extern "C"
