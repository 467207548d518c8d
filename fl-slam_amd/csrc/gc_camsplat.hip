// gc_camsplat.hip — camera splats on the device: the LiDAR depth evidence of every camera feature, the
// product-of-experts depth fusion, and the camera slice of a MeasurementBatch.
//
//  points base -> camera, splat_prep_fused, base-frame loop     backend/backend_node.py:1872-1925
//  _project_camera, Route A, Route B, lidar_depth_evidence      frontend/sensors/lidar_camera_depth_fusion.py:80-442
//  backproject_camera, backprojection_cov_camera                :450-489
//  splat_prep_fused (PoE fusion, the two fall-backs)            frontend/sensors/splat_prep.py:37-134
//  feature_list_to_camera_batch                                 backend/camera_batch_utils.py:23-86
//  measurement_batch_from_camera_splats                         backend/structures/measurement_batch.py:165-259
//
// Three kernels, f64, no floating-point atomics and no slot claiming: every candidate list, every sum
// and every row has a fixed order, so the outputs are bitwise the same from run to run.
//
//  k_cs_project  one lane per point: the optional base -> camera transform, the projection exactly as
//                _project_camera writes it (division by z + 1e-12), (u, v) and the camera-frame point to
//                scratch. A point with z > 0 false (NaN included) gets u = v = NaN, so no radius test
//                ever takes it. The number of z > 0 points (an integer) goes to a device word.
//  k_cs_query    one 256-thread workgroup per query. Each of the four waves scans its own contiguous
//                quarter of the points in index order and compacts the in-radius ones (ballot ranks)
//                into a list of its own; the four lists one after the other are the candidates in
//                ascending point index, whatever the scheduling. Route A: the median of z and of
//                |z - median| by an LDS bitonic sort, the mean and the population variance by
//                fixed-order sums (block_sum, gc_blocksum.h). Route B: a bitonic sort by (squared
//                distance to the ray, candidate position), the first k_use of it one per thread, the weighted centroid and scatter by
//                fixed-order sums, eigh3, the ray-plane intersection and the reliabilities.
//  k_cs_finish   one lane per row: the PoE fusion with its fall-backs, the backprojection and its
//                closed-form covariance, the base-frame transform, Λ = inv3(Σ + eps_lift I), θ = Λ μ, the
//                vMF lobe, colour, weight, timestamp, source, index and mask; rows from n_valid to
//                n_total are zeroed. gc_measurement_batch_from_camera_splats runs the same kernel from
//                given positions and covariances.
#include <hip/hip_runtime.h>
#include <string>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"

namespace gc {
namespace {

constexpr int kCsT = 256;                      // threads per workgroup
constexpr int kCsWaves = kCsT / 64;
constexpr int kCsMaxNear = GC_CAM_MAX_NEAR;    // in-radius candidates a query holds in LDS
constexpr int kCsMaxK = GC_CAM_MAX_FIT_POINTS;  // lidar_ray_plane_fit_max_points: one fitted point per thread
constexpr int kCsUnroll = 8;                   // 64-point chunks in flight per wave
constexpr int64_t kCsMaxPoints = GC_CAM_MAX_POINTS;
constexpr int64_t kCsMaxQueries = GC_CAM_MAX_QUERIES;
static_assert(kCsMaxK == kCsT, "the plane fit holds one selected point per thread");

struct CsIntr { double fx, fy, cx, cy; };
struct CsXf { int has; double R[9], t[3]; };  // x_base = R x_cam + t
struct CsCfg {
  double w_cam, w_lidar, gamma, radius, base_sigma, var_min, n0, alpha_cnt, beta_mad, gamma_repr, delta, alpha,
      t_angle, beta, rho0, gamma_res, eps, z_min, sigma_max_sq, alpha_z;
  int min_points, max_points;
};

// _softplus (:197-204): the cut-offs at +-20 and log(1 + exp(x)) between them
GC_DEV double cs_softplus(double x) {
  if (x > 20.0) return x;
  if (x < -20.0) return 0.0;
  return log(1.0 + exp(x));
}

GC_DEV bool cs_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }  // false for NaN

__global__ void __launch_bounds__(kCsT) k_cs_project(int64_t N, const double* __restrict__ pts, CsXf xf, CsIntr K,
                                                     double2* __restrict__ uv, double* __restrict__ pcam,
                                                     int32_t* __restrict__ n_front) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kCsT + threadIdx.x;
  bool front = false;
  if (i < N) {
    double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (xf.has) {  // p_cam = Rᵀ (p - t) (backend_node.py:1876)
      const double d0 = x - xf.t[0], d1 = y - xf.t[1], d2 = z - xf.t[2];
      x = xf.R[0] * d0 + xf.R[3] * d1 + xf.R[6] * d2;
      y = xf.R[1] * d0 + xf.R[4] * d1 + xf.R[7] * d2;
      z = xf.R[2] * d0 + xf.R[5] * d1 + xf.R[8] * d2;
    }
    front = z > 0.0;
    const double zz = z + 1e-12, nan = __builtin_nan("");
    const double u = K.fx * (x / zz) + K.cx, v = K.fy * (y / zz) + K.cy;  // :93-94
    uv[i] = front ? make_double2(u, v) : make_double2(nan, nan);
    pcam[3 * i] = x;
    pcam[3 * i + 1] = y;
    pcam[3 * i + 2] = z;
  }
  const unsigned long long b = __ballot(front);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_front, __popcll(b));  // an integer count: any order
}

// ascending bitonic sort of P (a power of two, <= kCsMaxNear) (key, val) pairs in LDS, val breaking ties
GC_DEV void cs_sort(unsigned long long* key, int32_t* val, int P) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int c = t; c < P / 2; c += kCsT) {
        const int i = 2 * j * (c / j) + (c % j), q = i + j;
        const bool up = (i & k) == 0;
        const unsigned long long a = key[i], b = key[q];
        const int32_t va = val[i], vb = val[q];
        const bool gt = a > b || (a == b && va > vb);
        if (gt == up) {
          key[i] = b; key[q] = a;
          val[i] = vb; val[q] = va;
        }
      }
      __syncthreads();
    }
}

// np.median of the n sorted non-negative doubles whose bit patterns are key[0..n)
GC_DEV double cs_median_sorted(const unsigned long long* key, int n) {
  const double hi = __longlong_as_double((long long)key[n / 2]);
  if (n & 1) return hi;
  return (__longlong_as_double((long long)key[n / 2 - 1]) + hi) / 2.0;
}

constexpr int kCsEv = GC_CAM_EV;  // Λ_A θ_A Λ_B θ_B Λ_ell θ_ell z*_B σ²_B w_B

__global__ void __launch_bounds__(kCsT) k_cs_query(int64_t N, const double2* __restrict__ uv,
                                                   const double* __restrict__ pcam, const double* __restrict__ pw,
                                                   const double* __restrict__ query, CsIntr K, CsCfg cfg,
                                                   const int32_t* __restrict__ n_front, double* __restrict__ ev,
                                                   int32_t* __restrict__ counts, int32_t* __restrict__ over) {
#pragma clang fp contract(off)
  __shared__ int32_t wl[kCsWaves][kCsMaxNear];
  __shared__ int wcnt[kCsWaves];
  __shared__ int32_t cidx[kCsMaxNear];
  __shared__ double cz[kCsMaxNear];
  __shared__ unsigned long long key[kCsMaxNear];
  __shared__ int32_t val[kCsMaxNear];
  __shared__ double red[kCsWaves * 6];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t m = blockIdx.x;
  const double uq = query[2 * m], vq = query[2 * m + 1];
  const double r2 = cfg.radius * cfg.radius, nan = __builtin_nan("");
  // ---- the in-radius candidates (:139-140, :294-295), this wave's quarter in index order
  {
    const int64_t seg = (N + 64 * kCsWaves - 1) / (64 * kCsWaves) * 64;
    const int64_t b0 = wv * seg, b1 = b0 + seg < N ? b0 + seg : N;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int cnt = 0;
    for (int64_t base = b0; base < b1; base += 64 * kCsUnroll) {
      double2 p[kCsUnroll];
#pragma unroll
      for (int u = 0; u < kCsUnroll; ++u) {
        const int64_t i = base + u * 64 + lane;
        p[u] = i < b1 ? uv[i] : make_double2(nan, nan);
      }
#pragma unroll
      for (int u = 0; u < kCsUnroll; ++u) {
        const double du = p[u].x - uq, dv = p[u].y - vq;
        const double d = du * du + dv * dv;
        const bool in = d <= r2;  // false for the NaN of a point not in front
        const unsigned long long b = __ballot(in);
        const int pos = cnt + __popcll(b & lt);
        if (in && pos < kCsMaxNear) wl[wv][pos] = (int32_t)(base + u * 64 + lane);
        cnt += __popcll(b);
      }
    }
    if (lane == 0) wcnt[wv] = cnt;
  }
  __syncthreads();
  int n = 0, off = 0;
  for (int u = 0; u < kCsWaves; ++u) {
    off += u < wv ? wcnt[u] : 0;
    n += wcnt[u];
  }
  double* e = ev + m * kCsEv;
  if (t == 0) counts[m] = n;
  const bool too_many = n > kCsMaxNear;
  if (too_many && t == 0) atomicMax(over, n);  // an integer maximum: any order
  if (too_many || n == 0 || n < cfg.min_points || n_front[0] < cfg.min_points) {
    // fewer than min_points candidates (:145, :301) or z > 0 points in all (:276): no LiDAR evidence
    if (t == 0) {
      for (int q = 0; q < 6; ++q) e[q] = 0.0;
      e[6] = nan; e[7] = nan; e[8] = 0.0;
    }
    return;
  }
  for (int j = lane; j < wcnt[wv]; j += 64) cidx[off + j] = wl[wv][j];
  __syncthreads();
  int P = 2;
  while (P < n) P <<= 1;
  // ---- Route A (:147-162)
  for (int j = t; j < P; j += kCsT) {
    double z = 0.0;
    if (j < n) {
      z = pcam[3 * (int64_t)cidx[j] + 2];
      cz[j] = z;
    }
    key[j] = j < n ? (unsigned long long)__double_as_longlong(z) : ~0ull;  // z > 0: the bits order as the values
    val[j] = j;
  }
  cs_sort(key, val, P);
  const double z_med = cs_median_sorted(key, n);
  __syncthreads();
  for (int j = t; j < P; j += kCsT) {
    key[j] = j < n ? (unsigned long long)__double_as_longlong(fabs(cz[j] - z_med)) : ~0ull;
    val[j] = j;
  }
  cs_sort(key, val, P);
  const double mad = cs_median_sorted(key, n);
  __syncthreads();
  double s1[1] = {0.0};
  for (int j = t; j < n; j += kCsT) s1[0] += cz[j];
  block_sum<1, kCsWaves>(s1, red);
  const double z_mean = s1[0] / (double)n;
  s1[0] = 0.0;
  for (int j = t; j < n; j += kCsT) {
    const double d = cz[j] - z_mean;
    s1[0] += d * d;
  }
  block_sum<1, kCsWaves>(s1, red);
  const double var_spread = n >= 2 ? s1[0] / (double)n : 0.0;  // np.var: the population variance
  const double sigma_A = 1.4826 * mad, sigma_A_sq = sigma_A * sigma_A;
  double sig_a = cfg.base_sigma * cfg.base_sigma + fmax(sigma_A_sq, var_spread);
  sig_a = fmax(sig_a, cfg.var_min);
  const double w_cnt = sigmoid(cfg.alpha_cnt * ((double)n - cfg.n0));
  const double w_mad = exp(-cfg.beta_mad * sigma_A_sq), w_repr = exp(-cfg.gamma_repr * var_spread);
  const double wA = w_cnt * w_mad * w_repr;
  double Lam_A = 0.0, th_A = 0.0;
  if (!(wA <= 0.0) && cs_finite(z_med) && !(z_med <= 0.0)) {
    Lam_A = wA / sig_a;
    th_A = Lam_A * z_med;
  }
  // ---- Route B (:293-347): the ray, the squared distances to it, the k_use nearest
  double ray[3];
  {
    const double dx = (uq - K.cx) / K.fx, dy = (vq - K.cy) / K.fy;
    const double nrm = sqrt(dx * dx + dy * dy + 1.0);
    if (nrm < 1e-12) { ray[0] = 0.0; ray[1] = 0.0; ray[2] = 1.0; }
    else { ray[0] = dx / nrm; ray[1] = dy / nrm; ray[2] = 1.0 / nrm; }
  }
  double rd[3];  // _distance_point_to_ray normalises once more (:189)
  {
    const double nr = sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]) + 1e-12;
    rd[0] = ray[0] / nr; rd[1] = ray[1] / nr; rd[2] = ray[2] / nr;
  }
  for (int j = t; j < P; j += kCsT) {
    unsigned long long kk = ~0ull;
    if (j < n) {
      const double* p = pcam + 3 * (int64_t)cidx[j];
      const double pl = p[0] * rd[0] + p[1] * rd[1] + p[2] * rd[2];
      const double e0 = p[0] - pl * rd[0], e1 = p[1] - pl * rd[1], e2 = p[2] - pl * rd[2];
      kk = (unsigned long long)__double_as_longlong(e0 * e0 + e1 * e1 + e2 * e2);
    }
    key[j] = kk;
    val[j] = j;
  }
  cs_sort(key, val, P);
  const int Kmax = min(cfg.max_points, n_front[0]);  // :280
  const int k_use = min(Kmax, n);
  // _fit_plane_weighted (:207-239): thread t holds the t-th nearest point
  double p[3] = {0.0, 0.0, 0.0}, w = 0.0;
  if (t < k_use) {
    const int64_t i = cidx[min(val[t], n - 1)];  // the padding sorts last: val[t] < n
    p[0] = pcam[3 * i]; p[1] = pcam[3 * i + 1]; p[2] = pcam[3 * i + 2];
    w = pw ? pw[i] : 1.0;
  }
  double a4[4] = {w, w * p[0], w * p[1], w * p[2]};
  block_sum<4, kCsWaves>(a4, red);
  const double sw = a4[0], w_sum = sw + 1e-300;
  const double cen[3] = {a4[1] / sw, a4[2] / sw, a4[3] / sw};
  const double c0 = p[0] - cen[0], c1 = p[1] - cen[1], c2 = p[2] - cen[2];
  double a6[6] = {w * c0 * c0, w * c0 * c1, w * c0 * c2, w * c1 * c1, w * c1 * c2, w * c2 * c2};
  if (!(t < k_use))
    for (int q = 0; q < 6; ++q) a6[q] = 0.0;  // cen may be NaN for an all-zero weight sum
  block_sum<6, kCsWaves>(a6, red);
  const double sxx = a6[0] / w_sum, sxy = a6[1] / w_sum, sxz = a6[2] / w_sum, syy = a6[3] / w_sum,
               syz = a6[4] / w_sum, szz = a6[5] / w_sum;
  const double S[9] = {sxx + 1e-12, sxy, sxz, sxy, syy + 1e-12, syz, sxz, syz, szz + 1e-12};
  double lam[3], V[9];
  eigh3(S, lam, V);
  // ascending eigenvalues; the normal is the eigenvector of the smallest
  int i0 = 0;
  if (lam[1] < lam[i0]) i0 = 1;
  if (lam[2] < lam[i0]) i0 = 2;
  double nrm[3] = {V[0], V[3], V[6]};
  if (i0 == 1) { nrm[0] = V[1]; nrm[1] = V[4]; nrm[2] = V[7]; }
  if (i0 == 2) { nrm[0] = V[2]; nrm[1] = V[5]; nrm[2] = V[8]; }
  const double la = i0 == 0 ? lam[1] : lam[0], lb = i0 == 2 ? lam[1] : lam[2];
  double lam2 = fmin(la, lb), lam3 = fmax(la, lb);
  if (nrm[2] < 0.0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
  const double res = c0 * nrm[0] + c1 * nrm[1] + c2 * nrm[2];
  s1[0] = t < k_use ? w * (res * res) : 0.0;
  block_sum<1, kCsWaves>(s1, red);
  const double sigma_perp_sq = fmax(s1[0] / sw, 0.0);
  if (t != 0) return;
  const double ndr = nrm[0] * ray[0] + nrm[1] * ray[1] + nrm[2] * ray[2];
  const double z_raw = (nrm[0] * cen[0] + nrm[1] * cen[1] + nrm[2] * cen[2]) / (ndr + cfg.delta);
  const double z_b = cs_softplus(z_raw - cfg.z_min) + cfg.z_min;
  const double w_behind = z_raw < cfg.z_min ? sigmoid(z_raw - cfg.z_min) : 1.0;
  const double ndr_sq = ndr * ndr + cfg.delta;
  double sig_b = cfg.base_sigma * cfg.base_sigma + sigma_perp_sq / fmax(ndr_sq, cfg.delta);
  sig_b = fmax(sig_b, cfg.var_min);
  sig_b = fmin(sig_b, cfg.sigma_max_sq);
  const double w_angle = sigmoid(cfg.alpha * (fabs(ndr) - cfg.t_angle));
  lam2 = fmax(lam2, cfg.eps);
  lam3 = fmax(lam3, cfg.eps);
  const double rho = lam2 / (lam3 + cfg.eps);
  const double w_planar = sigmoid(cfg.beta * (rho - cfg.rho0));
  const double w_res = exp(-cfg.gamma_res * sigma_perp_sq);
  double w_plane = w_angle * w_planar * w_res * w_behind;
  const double w_z = sigmoid(cfg.alpha_z * (z_b - cfg.z_min));
  w_plane = w_plane * w_z;
  const double w_b = w_plane > 0.0 ? w_plane : (w_plane == w_plane ? 0.0 : w_plane);  // max(w, 0.0), NaN kept
  // _route_b_natural_params (:377-385)
  double Lam_B = 0.0, th_B = 0.0;
  if (cs_finite(z_b) && z_b > 0.0 && cs_finite(sig_b) && sig_b > 0.0 && w_b > 0.0) {
    Lam_B = w_b / fmax(sig_b, cfg.var_min);
    th_B = Lam_B * z_b;
  }
  e[0] = Lam_A; e[1] = th_A; e[2] = Lam_B; e[3] = th_B;
  e[4] = (Lam_A + Lam_B) * cfg.gamma;  // :428-433 (a gamma of 1 changes nothing)
  e[5] = (th_A + th_B) * cfg.gamma;
  e[6] = z_b; e[7] = sig_b; e[8] = w_b;
}

struct CsFin {
  int tail;  // 0: fuse features with the evidence; 1: rows from given positions, covariances, directions
  int64_t M;
  int n_feat, n_total, n_lobes;
  double eps_lift, ts, pixel_var, w_cam, w_lidar, var_min;
  CsIntr K;
  CsXf xf;
  const double *uv, *Lc, *thc, *weight, *kappa, *mu, *color, *xyz, *cov, *ev, *tstamps;
  const uint8_t *has_mu, *has_color;
  double *fxyz, *fcov;
  uint8_t* fflag;
  double *Lam, *tht, *eta, *wts, *tst, *col;
  int32_t *src, *sidx;
  uint8_t* valid;
};

__global__ void __launch_bounds__(kCsT) k_cs_finish(CsFin a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kCsT + threadIdx.x;
  const int64_t n_valid = a.M < a.n_feat ? a.M : a.n_feat;
  double pos[3], cv[9], dir[3];
  if (i < a.M) {
    if (a.tail) {
#pragma unroll
      for (int q = 0; q < 3; ++q) { pos[q] = a.xyz[3 * i + q]; dir[q] = a.mu[3 * i + q]; }
#pragma unroll
      for (int q = 0; q < 9; ++q) cv[q] = a.cov[9 * i + q];
    } else {
      // splat_prep.py:73-101
      const double u = a.uv[2 * i], v = a.uv[2 * i + 1];
      const double Lam_f = a.w_cam * a.Lc[i] + a.w_lidar * a.ev[kCsEv * i + 4];
      const double th_f = a.w_cam * a.thc[i] + a.w_lidar * a.ev[kCsEv * i + 5];
      bool fused = !(Lam_f <= 0.0) && cs_finite(Lam_f) && cs_finite(th_f);
      double z_f = 0.0, sig_f = 0.0;
      if (fused) {
        z_f = th_f / Lam_f;
        sig_f = 1.0 / Lam_f;
        fused = cs_finite(z_f) && !(z_f <= 0.0) && cs_finite(sig_f) && !(sig_f <= 0.0);
      }
      if (fused) {
        const double var_z = fmax(sig_f, a.var_min);
        const double du = u - a.K.cx, dv = v - a.K.cy;
        pos[0] = du * z_f / a.K.fx;  // :452-454
        pos[1] = dv * z_f / a.K.fy;
        pos[2] = z_f;
        const double vu = fmax(a.pixel_var, 0.0), vv = vu, vz = fmax(var_z, 0.0);  // :473-489
        const double var_x = (z_f * z_f * vu + du * du * vz + vu * vz) / (a.K.fx * a.K.fx);
        const double var_y = (z_f * z_f * vv + dv * dv * vz + vv * vz) / (a.K.fy * a.K.fy);
        const double cxy = (du * dv * vz) / (a.K.fx * a.K.fy), cxz = (du * vz) / a.K.fx, cyz = (dv * vz) / a.K.fy;
        cv[0] = var_x; cv[1] = cxy; cv[2] = cxz;
        cv[3] = cxy; cv[4] = var_y; cv[5] = cyz;
        cv[6] = cxz; cv[7] = cyz; cv[8] = vz;
      } else {  // the unfused feature as it came (:85-93)
#pragma unroll
        for (int q = 0; q < 3; ++q) pos[q] = a.xyz[3 * i + q];
#pragma unroll
        for (int q = 0; q < 9; ++q) cv[q] = a.cov[9 * i + q];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) a.fxyz[3 * i + q] = pos[q];
#pragma unroll
      for (int q = 0; q < 9; ++q) a.fcov[9 * i + q] = cv[q];
      a.fflag[i] = fused ? 1 : 0;
      const bool has_mu = a.has_mu[i] != 0;
      double mu[3] = {0.0, 0.0, 0.0};
      if (has_mu)
        for (int q = 0; q < 3; ++q) mu[q] = a.mu[3 * i + q];
      if (a.xf.has) {  // backend_node.py:1892-1899
        double pb[3], t1[9], t2[9], mb[3];
        mat3_vec(a.xf.R, pos, pb);
        for (int q = 0; q < 3; ++q) pos[q] = pb[q] + a.xf.t[q];
        mat3_mul(a.xf.R, cv, t1);
        mat3_mul_nt(t1, a.xf.R, t2);
        for (int q = 0; q < 9; ++q) cv[q] = t2[q];
        mat3_vec(a.xf.R, mu, mb);
        for (int q = 0; q < 3; ++q) mu[q] = mb[q];
      }
      // camera_batch_utils.py:58-65
      const double d0 = has_mu ? mu[0] : pos[0], d1 = has_mu ? mu[1] : pos[1], d2 = has_mu ? mu[2] : pos[2];
      const double nd = sqrt(d0 * d0 + d1 * d1 + d2 * d2) + 1e-12;
      dir[0] = d0 / nd; dir[1] = d1 / nd; dir[2] = d2 / nd;
    }
  }
  if (i >= a.n_total) return;
  if (i < n_valid) {
    // measurement_batch.py:203-243
    double Sg[9], L[9], th[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) Sg[q] = cv[q] + ((q % 4 == 0) ? a.eps_lift : 0.0);
    inv3(Sg, L);
    mat3_vec(L, pos, th);
    const double kap = a.kappa[i];
#pragma unroll
    for (int q = 0; q < 9; ++q) a.Lam[9 * i + q] = L[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      a.tht[3 * i + q] = th[q];
      a.eta[(i * a.n_lobes) * 3 + q] = kap * dir[q];
      const bool hc = a.color && (a.tail || a.has_color[i] != 0);
      a.col[3 * i + q] = hc ? fmin(fmax(a.color[3 * i + q], 0.0), 1.0) : 0.5;
    }
    for (int q = 3; q < 3 * a.n_lobes; ++q) a.eta[(i * a.n_lobes) * 3 + q] = 0.0;
    a.wts[i] = a.weight[i];
    a.tst[i] = a.tail ? a.tstamps[i] : a.ts;
    a.src[i] = 0;
    a.sidx[i] = (int32_t)i;
    a.valid[i] = 1;
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) a.Lam[9 * i + q] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      a.tht[3 * i + q] = 0.0;
      a.col[3 * i + q] = 0.0;
    }
    for (int q = 0; q < 3 * a.n_lobes; ++q) a.eta[(i * a.n_lobes) * 3 + q] = 0.0;
    a.wts[i] = 0.0;
    a.tst[i] = 0.0;
    a.src[i] = 0;
    a.sidx[i] = 0;
    a.valid[i] = 0;
  }
}

int cs_parse_cfg(gc_ctx* ctx, const gc_cam_cfg* h, CsCfg* c) {
  GC_CHECK_ARG(ctx, cfg_all<23>(h, [](double v) { return v == v; }), "NaN in the configuration");
  GC_CHECK_ARG(ctx, h->lidar_projection_radius_pix > 0.0 && h->lidar_projection_radius_pix <= 1e300,
               "lidar_projection_radius_pix must be > 0 and finite");
  const double mp = h->lidar_plane_fit_min_points, k = h->lidar_ray_plane_fit_max_points;
  GC_CHECK_ARG(ctx, mp >= 1.0 && mp <= 16777216.0 && mp == floor(mp), "lidar_plane_fit_min_points must be an integer >= 1");
  GC_CHECK_ARG(ctx, k >= 1.0 && k <= (double)kCsMaxK && k == floor(k),
               "lidar_ray_plane_fit_max_points must be an integer in [1, 256]");
  c->w_cam = h->depth_fusion_weight_camera; c->w_lidar = h->depth_fusion_weight_lidar; c->gamma = h->gamma_lidar;
  c->radius = h->lidar_projection_radius_pix; c->min_points = (int)mp; c->base_sigma = h->lidar_depth_base_sigma_m;
  c->var_min = h->depth_var_min_m2; c->n0 = h->point_support_n0; c->alpha_cnt = h->point_support_alpha;
  c->beta_mad = h->spread_mad_beta; c->gamma_repr = h->repr_gamma; c->max_points = (int)k;
  c->delta = h->plane_intersection_delta; c->alpha = h->plane_angle_sigmoid_alpha;
  c->t_angle = h->plane_angle_sigmoid_t; c->beta = h->plane_planarity_sigmoid_beta;
  c->rho0 = h->plane_planarity_rho0; c->gamma_res = h->plane_residual_exp_gamma; c->eps = h->plane_fit_eps;
  c->z_min = h->depth_min_m; c->sigma_max_sq = h->depth_sigma_max_sq; c->alpha_z = h->depth_min_sigmoid_alpha_z;
  return GC_OK;
}

int cs_parse_intr(gc_ctx* ctx, const double* k4, CsIntr* K) {
  for (int q = 0; q < 4; ++q) GC_CHECK_ARG(ctx, fabs(k4[q]) <= 1e300, "the intrinsics must be finite");
  GC_CHECK_ARG(ctx, k4[0] != 0.0 && k4[1] != 0.0, "fx and fy must not be 0");
  K->fx = k4[0]; K->fy = k4[1]; K->cx = k4[2]; K->cy = k4[3];
  return GC_OK;
}

int cs_parse_xf(gc_ctx* ctx, const double* R, const double* t, CsXf* xf) {
  GC_CHECK_ARG(ctx, (R == nullptr) == (t == nullptr), "R and t must be given together");
  xf->has = R != nullptr;
  for (int q = 0; q < 9; ++q) xf->R[q] = R ? R[q] : (q % 4 == 0 ? 1.0 : 0.0);
  for (int q = 0; q < 3; ++q) xf->t[q] = t ? t[q] : 0.0;
  for (int q = 0; q < 9; ++q) GC_CHECK_ARG(ctx, fabs(xf->R[q]) <= 1e300, "R must be finite");
  for (int q = 0; q < 3; ++q) GC_CHECK_ARG(ctx, fabs(xf->t[q]) <= 1e300, "t must be finite");
  return GC_OK;
}

struct CsScratch {
  double2* uv;
  double* pcam;
  int32_t* words;  // [0] the number of z > 0 points, [1] the largest candidate count above the cap
};

int cs_scratch(gc_ctx* ctx, int64_t N, CsScratch* s) {
  const size_t npt = (size_t)(N > 0 ? N : 1);
  return gc::carve_scratch(ctx, [&](gc::Carver& c) {
    s->uv = c.take<double2>(npt);
    s->pcam = c.take<double>(3 * npt);
    s->words = c.take<int32_t>(2);
  });
}

// project and query: the evidence rows (M, GC_CAM_EV) and the in-radius counts (M)
int cs_evidence(gc_ctx* ctx, int64_t N, const double* d_points, const CsXf& xf, int64_t M, const double* d_uv,
                const CsIntr& K, const CsCfg& cfg, const double* d_pw, const CsScratch& s, double* d_ev,
                int32_t* d_counts) {
  hipStream_t st = ctx->stream;
  GC_HIP(ctx, hipMemsetAsync(s.words, 0, 2 * sizeof(int32_t), st));
  if (N > 0) {
    hipLaunchKernelGGL(k_cs_project, dim3((unsigned)((N + kCsT - 1) / kCsT)), dim3(kCsT), 0, st, N, d_points, xf, K,
                       s.uv, s.pcam, s.words);
    GC_LAUNCH_CHECK(ctx);
  }
  if (M > 0) {
    hipLaunchKernelGGL(k_cs_query, dim3((unsigned)M), dim3(kCsT), 0, st, N, (const double2*)s.uv,
                       (const double*)s.pcam, d_pw, d_uv, K, cfg, (const int32_t*)s.words, d_ev, d_counts,
                       s.words + 1);
    GC_LAUNCH_CHECK(ctx);
  }
  return GC_OK;
}

// the one wait of an entry: the candidate-cap word
int cs_check_cap(gc_ctx* ctx, const CsScratch& s) {
  int32_t over = 0;
  GC_HIP(ctx, hipMemcpyAsync(&over, s.words + 1, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (int rc_w = gc::wait_stream(ctx, ctx->stream, "the camera splat evidence")) return rc_w;
  if (over > 0) {
    gc::set_error(ctx, "invalid argument: a query has " + std::to_string(over) +
                           " LiDAR points inside lidar_projection_radius_pix; at most GC_CAM_MAX_NEAR = " +
                           std::to_string(kCsMaxNear) + " are supported");
    return GC_ERR_ARG;
  }
  return GC_OK;
}

int cs_check_budget(gc_ctx* ctx, int32_t n_feat, int32_t n_surfel, int32_t n_lobes) {
  GC_CHECK_ARG(ctx, n_feat >= 0 && n_feat <= (1 << 24), "n_feat must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, n_surfel >= 0 && n_surfel <= (1 << 24), "n_surfel must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, n_lobes >= 1 && n_lobes <= 8, "n_lobes must be in [1, 8]");
  return GC_OK;
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_lidar_depth_evidence(gc_ctx* ctx, int64_t N, const double* d_points_cam, int64_t M, const double* d_uv,
                                const double* h_intrinsics, const gc_cam_cfg* h, const double* d_point_weights,
                                double* d_evidence, int32_t* d_counts) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, h_intrinsics && h, "NULL argument");
  GC_CHECK_ARG(ctx, N >= 0 && N <= kCsMaxPoints, "N must be in [0, 4194304]");
  GC_CHECK_ARG(ctx, M >= 0 && M <= kCsMaxQueries, "M must be in [0, 4096]");
  GC_CHECK_ARG(ctx, N == 0 || d_points_cam, "NULL point buffer");
  GC_CHECK_ARG(ctx, M == 0 || (d_uv && d_evidence && d_counts), "NULL query or output buffer");
  CsCfg cfg;
  CsIntr K;
  CsXf xf;
  if (int rc = cs_parse_cfg(ctx, h, &cfg)) return rc;
  if (int rc = cs_parse_intr(ctx, h_intrinsics, &K)) return rc;
  if (int rc = cs_parse_xf(ctx, nullptr, nullptr, &xf)) return rc;
  if (M == 0) return GC_OK;
  CsScratch s;
  if (int rc = cs_scratch(ctx, N, &s)) return rc;
  if (int rc = cs_evidence(ctx, N, d_points_cam, xf, M, d_uv, K, cfg, d_point_weights, s, d_evidence, d_counts))
    return rc;
  return cs_check_cap(ctx, s);
}

int32_t gc_camera_measurement_batch(gc_ctx* ctx, int64_t N, const double* d_points_base, const double* h_R9,
                                    const double* h_t3, int64_t M, const double* d_uv, const double* d_Lambda_c,
                                    const double* d_theta_c, const double* d_weight, const double* d_kappa,
                                    const double* d_mu_app, const uint8_t* d_has_mu_app, const double* d_color,
                                    const uint8_t* d_has_color, const double* d_xyz, const double* d_cov_xyz,
                                    const double* h_intrinsics, const gc_cam_cfg* h, double pixel_sigma,
                                    double timestamp_sec, int32_t n_feat, int32_t n_surfel, int32_t n_lobes,
                                    double eps_lift, double* d_Lambdas, double* d_thetas, double* d_etas,
                                    double* d_weights_out, int32_t* d_sources, int32_t* d_source_indices,
                                    uint8_t* d_valid_mask, double* d_timestamps_out, double* d_colors,
                                    double* d_fused_xyz, double* d_fused_cov, uint8_t* d_fused_flag,
                                    double* d_evidence, int32_t* d_counts) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, h_intrinsics && h, "NULL argument");
  GC_CHECK_ARG(ctx, N >= 0 && N <= kCsMaxPoints, "N must be in [0, 4194304]");
  GC_CHECK_ARG(ctx, M >= 0 && M <= kCsMaxQueries, "M must be in [0, 4096]");
  GC_CHECK_ARG(ctx, N == 0 || d_points_base, "NULL point buffer");
  GC_CHECK_ARG(ctx, M == 0 || (d_uv && d_Lambda_c && d_theta_c && d_weight && d_kappa && d_mu_app && d_has_mu_app &&
                               d_color && d_has_color && d_xyz && d_cov_xyz), "NULL feature buffer");
  GC_CHECK_ARG(ctx, M == 0 || (d_fused_xyz && d_fused_cov && d_fused_flag && d_evidence && d_counts),
               "NULL per-feature output buffer");
  GC_CHECK_ARG(ctx, d_Lambdas && d_thetas && d_etas && d_weights_out && d_sources && d_source_indices &&
                        d_valid_mask && d_timestamps_out && d_colors, "NULL batch buffer");
  if (int rc = cs_check_budget(ctx, n_feat, n_surfel, n_lobes)) return rc;
  GC_CHECK_ARG(ctx, pixel_sigma == pixel_sigma && timestamp_sec == timestamp_sec && eps_lift == eps_lift,
               "NaN scalar argument");
  CsCfg cfg;
  CsFin a = {};
  if (int rc = cs_parse_cfg(ctx, h, &cfg)) return rc;
  if (int rc = cs_parse_intr(ctx, h_intrinsics, &a.K)) return rc;
  if (int rc = cs_parse_xf(ctx, h_R9, h_t3, &a.xf)) return rc;
  const int64_t n_total = (int64_t)n_feat + n_surfel;
  CsScratch s;
  if (int rc = cs_scratch(ctx, N, &s)) return rc;
  if (int rc = cs_evidence(ctx, N, d_points_base, a.xf, M, d_uv, a.K, cfg, nullptr, s, d_evidence, d_counts)) return rc;
  a.tail = 0; a.M = M; a.n_feat = n_feat; a.n_total = (int)n_total; a.n_lobes = n_lobes;
  a.eps_lift = eps_lift; a.ts = timestamp_sec; a.pixel_var = pixel_sigma * pixel_sigma;
  a.w_cam = cfg.w_cam; a.w_lidar = cfg.w_lidar; a.var_min = cfg.var_min;
  a.uv = d_uv; a.Lc = d_Lambda_c; a.thc = d_theta_c; a.weight = d_weight; a.kappa = d_kappa; a.mu = d_mu_app;
  a.color = d_color; a.xyz = d_xyz; a.cov = d_cov_xyz; a.ev = d_evidence; a.tstamps = nullptr;
  a.has_mu = d_has_mu_app; a.has_color = d_has_color;
  a.fxyz = d_fused_xyz; a.fcov = d_fused_cov; a.fflag = d_fused_flag;
  a.Lam = d_Lambdas; a.tht = d_thetas; a.eta = d_etas; a.wts = d_weights_out; a.tst = d_timestamps_out;
  a.col = d_colors; a.src = d_sources; a.sidx = d_source_indices; a.valid = d_valid_mask;
  const int64_t rows = M > n_total ? M : n_total;
  if (rows > 0) {
    hipLaunchKernelGGL(k_cs_finish, dim3((unsigned)((rows + kCsT - 1) / kCsT)), dim3(kCsT), 0, ctx->stream, a);
    GC_LAUNCH_CHECK(ctx);
  }
  return cs_check_cap(ctx, s);
}

int32_t gc_measurement_batch_from_camera_splats(gc_ctx* ctx, int64_t N, const double* d_positions,
                                                const double* d_covariances, const double* d_directions,
                                                const double* d_kappas, const double* d_weights,
                                                const double* d_timestamps, const double* d_colors_in,
                                                int32_t n_feat, int32_t n_surfel, int32_t n_lobes, double eps_lift,
                                                double* d_Lambdas, double* d_thetas, double* d_etas,
                                                double* d_weights_out, int32_t* d_sources,
                                                int32_t* d_source_indices, uint8_t* d_valid_mask,
                                                double* d_timestamps_out, double* d_colors) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, N >= 0 && N <= ((int64_t)1 << 24), "N must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, N == 0 || (d_positions && d_covariances && d_directions && d_kappas && d_weights && d_timestamps),
               "NULL splat buffer");
  GC_CHECK_ARG(ctx, d_Lambdas && d_thetas && d_etas && d_weights_out && d_sources && d_source_indices &&
                        d_valid_mask && d_timestamps_out && d_colors, "NULL batch buffer");
  if (int rc = cs_check_budget(ctx, n_feat, n_surfel, n_lobes)) return rc;
  GC_CHECK_ARG(ctx, eps_lift == eps_lift, "NaN scalar argument");
  CsFin a = {};
  const int64_t n_total = (int64_t)n_feat + n_surfel;
  a.tail = 1; a.M = N < n_feat ? N : n_feat;  // rows past n_feat are never read
  a.n_feat = n_feat; a.n_total = (int)n_total; a.n_lobes = n_lobes; a.eps_lift = eps_lift;
  a.weight = d_weights; a.kappa = d_kappas; a.mu = d_directions; a.color = d_colors_in; a.xyz = d_positions;
  a.cov = d_covariances; a.tstamps = d_timestamps;
  a.Lam = d_Lambdas; a.tht = d_thetas; a.eta = d_etas; a.wts = d_weights_out; a.tst = d_timestamps_out;
  a.col = d_colors; a.src = d_sources; a.sidx = d_source_indices; a.valid = d_valid_mask;
  if (n_total > 0) {
    hipLaunchKernelGGL(k_cs_finish, dim3((unsigned)((n_total + kCsT - 1) / kCsT)), dim3(kCsT), 0, ctx->stream, a);
    GC_LAUNCH_CHECK(ctx);
  }
  return GC_OK;
}

}  // extern "C"
