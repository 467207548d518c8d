// gc_depthsurfel.hip — RGB-D surfel extraction on the device: coloured rows of the camera slice (source 0)
// of a MeasurementBatch from one depth image and, optionally, its rgb image. The operator is this build's
// (the reference's camera path is ORB-only); its semantics are stated at gc_extract_depth_surfels in
// include/gcslam.h and in DESIGN.md §4, "Depth surfels". The plane fit and the row are the LiDAR
// extractor's, restated below.
//
// Two kernels, f64, no floating-point atomics and no slot claiming: every sum and every row has a fixed
// order, so a batch is bitwise the same from run to run.
//
//  k_ds_fit    one wave per cell_px x cell_px cell, four cells per workgroup, no LDS and no barrier. Lane l
//              takes the cell's pixels l, l + 64, ... in row-major order within the cell (at most 16 at
//              cell_px = 32) and keeps their depths and validity in registers across the two passes: the
//              sums n, Σ p, Σ z, Σ rgb, then Σ (p - mean)(p - mean)ᵀ, lane-local in that order, then an xor
//              butterfly gives every lane the totals. Lane 0 runs the fit and the gates and writes the cell's
//              record and flag. A cell row is one contiguous run of cell_px float32 depths; the rgb is read
//              only where the depth is used.
//  k_ds_write  one lane per cell: the prefix sum of the validity flags in ascending cell id, as k_sf_write
//              does it, and the total V (integers: any order gives the same count), which every workgroup
//              adds up for itself; then the even selection, the rows, the slot -> cell record and the count.
#include <hip/hip_runtime.h>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"

namespace gc {
namespace {

// ---- The tail of _fit_one_cell and the batch row, restated from k_sf_fit (gc_surfel.hip), which keeps its
// own copy: with the LiDAR extractor moved onto one shared function its Lambdas and thetas came out of the
// device differing in the last bits from the build before ("Depth surfels"), and those bits are
// to stay. Same lines, same order.
//  _normalize, basis, _fit_one_cell from `cov = ... + eig_min I` on   backend/operators/lidar_surfel_extraction.py:69-81, :128-162
//  measurement_batch_add_lidar_surfels (info form, vMF lobe, grey)     backend/structures/measurement_batch.py:299-312
constexpr int kDsFitRec = 18;        // Λ_row (9) | θ (3) | κ n (3) | w | t | grey
constexpr double kDsEps = 1e-12;     // _fit_one_cell's eps default (:99), _normalize's eps (:69)

struct DsFitCfg {
  double nu, psi, kappa_scale, kappa_min, kappa_max, eig_min, eps_lift;
};

GC_DEV void ds_normalize(double* v) {  // _normalize (:69-70)
  const double n = norm3(v) + kDsEps;
  v[0] /= n; v[1] /= n; v[2] /= n;
}

GC_DEV void ds_sym_lift(double* A, double lift) {  // 0.5 (A + Aᵀ) + lift I
  const double a01 = 0.5 * (A[1] + A[3]), a02 = 0.5 * (A[2] + A[6]), a12 = 0.5 * (A[5] + A[7]);
  A[1] = a01; A[3] = a01; A[2] = a02; A[6] = a02; A[5] = a12; A[7] = a12;
  A[0] += lift; A[4] += lift; A[8] += lift;
}

// The plane of a cell from Cr, its covariance about the centroid (row-major, symmetric, unlifted), and the
// sensor's variance per axis: n the normal (n_z >= 0), *l0 the smallest eigenvalue of Cr + eig_min I, S the
// regularised covariance Σ_reg, *kappa the concentration of the vMF lobe.
GC_DEV void ds_plane_fit(const double* Cr, double sensor_var, const DsFitCfg& cfg, double* n, double* l0_out,
                         double* S, double* kappa) {
  double cov[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) cov[q] = Cr[q] + ((q % 4 == 0) ? cfg.eig_min : 0.0);
  // :128-131 — the eigenvector of the smallest eigenvalue, n_z >= 0, normalised
  double ev[3], V[9];
  eigh3(cov, ev, V);
  double l0 = ev[0];
  n[0] = V[0]; n[1] = V[3]; n[2] = V[6];
  if (ev[1] < l0) { l0 = ev[1]; n[0] = V[1]; n[1] = V[4]; n[2] = V[7]; }
  if (ev[2] < l0) { l0 = ev[2]; n[0] = V[2]; n[1] = V[5]; n[2] = V[8]; }
  if (n[2] < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
  ds_normalize(n);
  // :72-81 — the basis takes the normal normalised once more
  double n2[3] = {n[0], n[1], n[2]};
  ds_normalize(n2);
  double e1[3], e2[3];
  if (fabs(n2[2]) < 0.9) { e1[0] = -n2[1]; e1[1] = n2[0]; e1[2] = 0.0; }
  else { e1[0] = -n2[2]; e1[1] = 0.0; e1[2] = n2[0]; }
  ds_normalize(e1);
  cross3(n2, e1, e2);
  ds_normalize(e2);
  // :134-140 — Σ w (d·e)² / w_sum = eᵀ C e with the unlifted C
  double Ce[3];
  mat3_vec(Cr, e1, Ce);
  const double var_e1 = dot3(e1, Ce) + sensor_var;
  mat3_vec(Cr, e2, Ce);
  const double var_e2 = dot3(e2, Ce) + sensor_var;
  const double sig_perp = fmax(l0, cfg.eig_min);
  const double var_perp = sig_perp + sensor_var;
  const double d1 = fmax(var_e1, cfg.eig_min), d2 = fmax(var_e2, cfg.eig_min), d3 = fmax(var_perp, cfg.eig_min);
  // :142-154 — Σ = V D Vᵀ, Wishart regularisation in precision space
  double Lm[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) S[3 * a + b] = d1 * e1[a] * e1[b] + d2 * e2[a] * e2[b] + d3 * n[a] * n[b];
  ds_sym_lift(S, cfg.eig_min);
  S[0] += cfg.eig_min; S[4] += cfg.eig_min; S[8] += cfg.eig_min;  // inv(Σ + eig_min I)
  inv3(S, Lm);
  ds_sym_lift(Lm, 0.0);
  const double wish = cfg.nu / fmax(cfg.psi, kDsEps);
  Lm[0] += wish; Lm[4] += wish; Lm[8] += wish;
  ds_sym_lift(Lm, cfg.eig_min);
  inv3(Lm, S);
  ds_sym_lift(S, cfg.eig_min);  // Σ_reg
  // :156-162
  *kappa = clampd(cfg.kappa_scale / sqrt(fmax(sig_perp, cfg.eig_min)), cfg.kappa_min, cfg.kappa_max);
  *l0_out = l0;
}

// measurement_batch.py:299-312 — the info form of the row at pos, the vMF lobe and the grey into r
// (kDsFitRec doubles); S (Σ_reg) is lifted in place.
GC_DEV void ds_fit_record(double* S, const double* pos, const double* n, double kappa, double w, double t,
                          double eps_lift, double* r) {
  double Lm[9], th[3];
  S[0] += eps_lift; S[4] += eps_lift; S[8] += eps_lift;
  inv3(S, Lm);
  mat3_vec(Lm, pos, th);
#pragma unroll
  for (int q = 0; q < 9; ++q) r[q] = Lm[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    r[9 + q] = th[q];
    r[12 + q] = kappa * n[q];
  }
  r[15] = w;
  r[16] = t;
  r[17] = 0.25 + 0.5 * (clampd(n[2], -1.0, 1.0) + 1.0) / 2.0;
}

// ---- the operator
constexpr int kDsT = 256;                   // threads per workgroup, both kernels
constexpr int kDsCellsPerWg = kDsT / 64;    // k_ds_fit: one wave per cell
constexpr int kDsMinCell = 4, kDsMaxCell = 32;
constexpr int kDsPerLane = kDsMaxCell * kDsMaxCell / 64;  // pixels a lane holds at cell_px = 32
constexpr int kDsRec = kDsFitRec + 2;       // Λ_row (9) | θ (3) | κ n (3) | w | t | r g b
constexpr int kDsMaxCells = GC_SURFEL_MAX_CELLS;
constexpr int kDsMaxAxis = 16384;

struct DsArgs {
  int H, W, cell_px, n_cx, n_cells, min_count, depth_model, n_feat, n_in, n_lobes;
  double fx, fy, cx, cy, R[9], t[3];
  double min_depth, max_depth, sigma0, slope, plane_gate, min_cos, weight_scale, timestamp;
};

// pixel (row i, column j) at depth z through its centre, in the base frame
GC_DEV void ds_point(const DsArgs& a, int i, int j, double z, double* p) {
  const double pc[3] = {z * ((j + 0.5 - a.cx) / a.fx), z * ((i + 0.5 - a.cy) / a.fy), z};
  mat3_vec(a.R, pc, p);
  p[0] += a.t[0]; p[1] += a.t[1]; p[2] += a.t[2];
}

__global__ void __launch_bounds__(kDsT) k_ds_fit(DsArgs a, DsFitCfg cfg, const float* __restrict__ depth,
                                                 const uint8_t* __restrict__ rgb, double* __restrict__ rec,
                                                 int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * kDsCellsPerWg + (threadIdx.x >> 6);
  if (c >= a.n_cells) return;  // the whole wave
  const int i0 = (c / a.n_cx) * a.cell_px, j0 = (c % a.n_cx) * a.cell_px, area = a.cell_px * a.cell_px;
  float z[kDsPerLane];
  unsigned used = 0u;
  double s1[4] = {0.0, 0.0, 0.0, 0.0};  // Σ p (3) | Σ z
  int cnt = 0, col[3] = {0, 0, 0};
#pragma unroll
  for (int q = 0; q < kDsPerLane; ++q) {
    z[q] = 0.0f;
    const int k = lane + 64 * q;
    if (k >= area) continue;
    const int i = i0 + k / a.cell_px, j = j0 + k % a.cell_px;
    if (i >= a.H || j >= a.W) continue;  // an edge cell's pixels outside the image are missing
    const int64_t px = (int64_t)i * a.W + j;
    const float zf = depth[px];
    const double zd = (double)zf;
    if (!(isfinite(zf) && zd > a.min_depth && zd < a.max_depth)) continue;
    z[q] = zf;
    used |= 1u << q;
    double p[3];
    ds_point(a, i, j, zd, p);
    s1[0] += p[0]; s1[1] += p[1]; s1[2] += p[2]; s1[3] += zd;
    cnt += 1;
    if (rgb) {
      col[0] += rgb[3 * px]; col[1] += rgb[3 * px + 1]; col[2] += rgb[3 * px + 2];
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s1[q] = group_sum_xor<64>(s1[q]);
  cnt = group_sum_xor<64>(cnt);
#pragma unroll
  for (int q = 0; q < 3; ++q) col[q] = group_sum_xor<64>(col[q]);
  if (cnt < a.min_count) {  // min_count >= 3: an empty cell too
    if (lane == 0) flag[c] = 0;
    return;
  }
  const double n = (double)cnt;
  const double mu[3] = {s1[0] / n, s1[1] / n, s1[2] / n}, zbar = s1[3] / n;
  double s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // xx xy xz yy yz zz
#pragma unroll
  for (int q = 0; q < kDsPerLane; ++q) {
    if (!(used & (1u << q))) continue;
    const int k = lane + 64 * q;
    double p[3];
    ds_point(a, i0 + k / a.cell_px, j0 + k % a.cell_px, (double)z[q], p);
    const double dx = p[0] - mu[0], dy = p[1] - mu[1], dz = p[2] - mu[2];
    s2[0] += dx * dx; s2[1] += dx * dy; s2[2] += dx * dz;
    s2[3] += dy * dy; s2[4] += dy * dz; s2[5] += dz * dz;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) s2[q] = group_sum_xor<64>(s2[q]);
  if (lane != 0) return;  // every lane holds the same totals: one fits and writes
  const double Cr[9] = {s2[0] / n, s2[1] / n, s2[2] / n, s2[1] / n, s2[3] / n, s2[4] / n, s2[2] / n, s2[4] / n, s2[5] / n};
  const double sigma = a.sigma0 + a.slope * (a.depth_model ? zbar * zbar : zbar);
  double nrm[3], l0, S[9], kappa;
  ds_plane_fit(Cr, sigma * sigma, cfg, nrm, &l0, S, &kappa);
  // the gates: a depth step inside the cell, a surface seen edge-on
  const double gate = a.plane_gate * sigma;
  const double ray[3] = {mu[0] - a.t[0], mu[1] - a.t[1], mu[2] - a.t[2]};
  const bool ok = (l0 - cfg.eig_min) <= gate * gate && fabs(dot3(nrm, ray)) / norm3(ray) >= a.min_cos;
  flag[c] = ok ? 1 : 0;
  if (!ok) return;
  double* r = rec + (int64_t)c * kDsRec;
  ds_fit_record(S, mu, nrm, kappa, a.weight_scale * n / (double)area, a.timestamp, cfg.eps_lift, r);
  if (rgb) {
#pragma unroll
    for (int q = 0; q < 3; ++q) r[17 + q] = (double)col[q] / (255.0 * n);
  } else {
    r[18] = r[17];
    r[19] = r[17];
  }
}

__global__ void __launch_bounds__(kDsT) k_ds_write(DsArgs a, const int32_t* __restrict__ flag,
                                                   const double* __restrict__ rec, double* __restrict__ Lam,
                                                   double* __restrict__ tht, double* __restrict__ eta,
                                                   double* __restrict__ wts, int32_t* __restrict__ src,
                                                   int32_t* __restrict__ sidx, uint8_t* __restrict__ valid,
                                                   double* __restrict__ tst, double* __restrict__ colr,
                                                   int32_t* __restrict__ slot_cells, int32_t* __restrict__ n_valid_out) {
  // One cell per thread. A workgroup counts the valid cells before its range and in all, then scans its own
  // 256 flags: `rank` is the cell's rank among the valid cells in ascending cell id.
  __shared__ int wbefore[kDsT / 64], wall[kDsT / 64], wtot[kDsT / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int first = blockIdx.x * kDsT, c = first + t;
  int before = 0, all = 0;
  for (int j = t; j < a.n_cells; j += kDsT) {
    const int fj = flag[j];
    all += fj;
    before += j < first ? fj : 0;
  }
  before = group_sum_xor<64>(before);
  all = group_sum_xor<64>(all);
  const int f = c < a.n_cells ? flag[c] : 0;
  int x = f;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 0) { wbefore[wv] = before; wall[wv] = all; }
  if (lane == 63) wtot[wv] = x;
  __syncthreads();
  int base = 0, pre = 0, V = 0;
  for (int u = 0; u < kDsT / 64; ++u) {
    base += wbefore[u];
    V += wall[u];
    pre += u < wv ? wtot[u] : 0;
  }
  const int64_t rank = base + pre + x - f, room = a.n_feat - a.n_in;
  const int n_keep = (int)(V <= room ? V : room);
  // V > room: rank r is kept iff floor((r + 1) room / V) > floor(r room / V); the kept before it are floor(r room / V)
  bool keep = f != 0;
  int64_t k = rank;
  if (f && V > room) {
    k = rank * room / V;
    keep = (rank + 1) * room / V > k;
  }
  if (keep) {
    const int64_t row = a.n_in + k;
    const double* r = rec + (int64_t)c * kDsRec;
    double v[kDsRec];
#pragma unroll
    for (int q = 0; q < kDsRec; ++q) v[q] = r[q];
#pragma unroll
    for (int q = 0; q < 9; ++q) Lam[9 * row + q] = v[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      tht[3 * row + q] = v[9 + q];
      eta[(row * a.n_lobes) * 3 + q] = v[12 + q];
      colr[3 * row + q] = v[17 + q];
    }
    for (int q = 3; q < 3 * a.n_lobes; ++q) eta[(row * a.n_lobes) * 3 + q] = 0.0;
    wts[row] = v[15];
    tst[row] = v[16];
    src[row] = 0;
    sidx[row] = (int32_t)row;
    valid[row] = 1;
    slot_cells[row] = c;
  }
  // the rows of [0, n_feat) this call does not write
  for (int64_t j = (int64_t)first + t; j < a.n_feat; j += (int64_t)gridDim.x * kDsT)
    if (j < a.n_in || j >= a.n_in + n_keep) slot_cells[j] = -1;
  if (blockIdx.x == 0 && t == 0) n_valid_out[0] = n_keep;
}

static_assert(kDsPerLane <= 32, "k_ds_fit keeps a lane's validity in one 32-bit word");

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_extract_depth_surfels(gc_ctx* ctx, const float* d_depth, const uint8_t* d_rgb8, int32_t H, int32_t W,
                                 const double* h_intrinsics, const double* h_R_base_camera, const double* h_t_base_camera,
                                 double timestamp_sec, int32_t n_camera_valid_in, const gc_surfel_cfg* h, int32_t cell_px,
                                 double min_fill, double min_depth, double max_depth, int32_t depth_model, double sigma0,
                                 double slope, double plane_gate, double min_cos_incidence, double weight_scale,
                                 double* d_Lambdas, double* d_thetas, double* d_etas, double* d_weights_out,
                                 int32_t* d_sources, int32_t* d_source_indices, uint8_t* d_valid_mask,
                                 double* d_timestamps_out, double* d_colors, int32_t* d_slot_cells, int32_t* h_n_valid) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, d_depth && h_intrinsics && h_R_base_camera && h_t_base_camera && h && d_slot_cells && h_n_valid,
               "NULL argument");
  GC_CHECK_ARG(ctx, d_Lambdas && d_thetas && d_etas && d_weights_out && d_sources && d_source_indices &&
                        d_valid_mask && d_timestamps_out && d_colors, "NULL batch buffer");
  GC_CHECK_ARG(ctx, H >= 1 && H <= kDsMaxAxis && W >= 1 && W <= kDsMaxAxis, "H and W must be in [1, 16384]");
  GC_CHECK_ARG(ctx, (int64_t)H * W <= (int64_t)GC_IMAGE_MAX_PIXELS, "H W must be at most GC_IMAGE_MAX_PIXELS");
  GC_CHECK_ARG(ctx, cell_px >= kDsMinCell && cell_px <= kDsMaxCell, "cell_px must be in [4, 32]");
  const int n_cx = (W + cell_px - 1) / cell_px, n_cy = (H + cell_px - 1) / cell_px;
  GC_CHECK_ARG(ctx, (int64_t)n_cx * n_cy <= kDsMaxCells, "the image must hold at most 16384 cells");
  const auto fin = [](double v) { return std::isfinite(v); };
  const double params[] = {timestamp_sec, min_fill, min_depth, max_depth, sigma0, slope, plane_gate, min_cos_incidence,
                           weight_scale, h->n_feat, h->n_surfel, h->wishart_nu, h->wishart_psi_scale, h->kappa_main_scale,
                           h->kappa_min, h->kappa_max, h->eig_min, h->eps_lift, h->n_lobes};
  GC_CHECK_ARG(ctx, std::all_of(std::begin(params), std::end(params), fin), "a non-finite parameter");
  GC_CHECK_ARG(ctx, std::all_of(h_intrinsics, h_intrinsics + 4, fin) && h_intrinsics[0] != 0.0 && h_intrinsics[1] != 0.0,
               "the intrinsics must be finite, fx and fy not 0");
  GC_CHECK_ARG(ctx, std::all_of(h_R_base_camera, h_R_base_camera + 9, fin) &&
                        std::all_of(h_t_base_camera, h_t_base_camera + 3, fin), "the extrinsics must be finite");
  const auto as_int = [](double v, double lo, double hi, int* out) {
    if (!(v >= lo && v <= hi) || v != floor(v)) return false;
    *out = (int)v;
    return true;
  };
  DsArgs a;
  int n_surfel;
  GC_CHECK_ARG(ctx, as_int(h->n_feat, 0, 1 << 24, &a.n_feat), "n_feat must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, as_int(h->n_surfel, 0, 1 << 24, &n_surfel), "n_surfel must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, as_int(h->n_lobes, 1, 8, &a.n_lobes), "n_lobes must be in [1, 8]");
  GC_CHECK_ARG(ctx, n_camera_valid_in >= 0 && n_camera_valid_in <= a.n_feat, "n_camera_valid_in must be in [0, n_feat]");
  GC_CHECK_ARG(ctx, min_fill > 0.0 && min_fill <= 1.0, "min_fill must be in (0, 1]");
  GC_CHECK_ARG(ctx, min_depth >= 0.0 && min_depth < max_depth, "the depth limits must satisfy 0 <= min_depth < max_depth");
  GC_CHECK_ARG(ctx, depth_model == 0 || depth_model == 1, "depth_model must be 0 or 1");
  GC_CHECK_ARG(ctx, sigma0 > 0.0 && slope >= 0.0, "sigma0 must be > 0 and slope >= 0");
  GC_CHECK_ARG(ctx, plane_gate > 0.0, "plane_gate must be > 0");
  GC_CHECK_ARG(ctx, min_cos_incidence >= 0.0 && min_cos_incidence < 1.0, "min_cos_incidence must be in [0, 1)");
  a.H = H; a.W = W; a.cell_px = cell_px; a.n_cx = n_cx; a.n_cells = n_cx * n_cy;
  const int fill = (int)ceil(min_fill * (double)(cell_px * cell_px));
  a.min_count = fill > 3 ? fill : 3;
  a.depth_model = depth_model; a.n_in = n_camera_valid_in;
  a.fx = h_intrinsics[0]; a.fy = h_intrinsics[1]; a.cx = h_intrinsics[2]; a.cy = h_intrinsics[3];
  for (int q = 0; q < 9; ++q) a.R[q] = h_R_base_camera[q];
  for (int q = 0; q < 3; ++q) a.t[q] = h_t_base_camera[q];
  a.min_depth = min_depth; a.max_depth = max_depth; a.sigma0 = sigma0; a.slope = slope; a.plane_gate = plane_gate;
  a.min_cos = min_cos_incidence; a.weight_scale = weight_scale; a.timestamp = timestamp_sec;
  const DsFitCfg cfg = {h->wishart_nu, h->wishart_psi_scale, h->kappa_main_scale, h->kappa_min, h->kappa_max,
                        h->eig_min, h->eps_lift};
  double* rec;
  int32_t *flag, *d_nv;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        rec = c.take<double>(kDsRec * (size_t)a.n_cells);
        flag = c.take<int32_t>(a.n_cells);
        d_nv = c.take<int32_t>(1);
      }))
    return rc;
  hipStream_t st = ctx->stream;
  const unsigned g_fit = (unsigned)((a.n_cells + kDsCellsPerWg - 1) / kDsCellsPerWg),
                 g_write = (unsigned)((a.n_cells + kDsT - 1) / kDsT);
  hipLaunchKernelGGL(k_ds_fit, dim3(g_fit), dim3(kDsT), 0, st, a, cfg, d_depth, d_rgb8, rec, flag);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_ds_write, dim3(g_write), dim3(kDsT), 0, st, a, (const int32_t*)flag, (const double*)rec,
                     d_Lambdas, d_thetas, d_etas, d_weights_out, d_sources, d_source_indices, d_valid_mask,
                     d_timestamps_out, d_colors, d_slot_cells, d_nv);
  GC_LAUNCH_CHECK(ctx);
  int32_t nv = 0;
  GC_HIP(ctx, hipMemcpyAsync(&nv, d_nv, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (int rc_w = gc::wait_stream(ctx, st, "the depth surfel count")) return rc_w;
  *h_n_valid = nv;
  return GC_OK;
}

}  // extern "C"
