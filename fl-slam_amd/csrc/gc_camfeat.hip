// gc_camfeat.hip — the image side of the camera features on the device: keypoints, the depth image and the
// colour image -> the arrays gc_camera_measurement_batch reads (gc_camsplat.hip).
//
//  safe_sigmoid, clamp                                          src/visual_feature_node.cpp:37-49
//  validate_depth, depth_weight, response_weight, depth_sigma   :184-226
//  depth_sample (nearest, median3, median5)                     :228-297
//  depth_sample_hex                                             :299-348
//  student_t_effective_var                                      :350-369
//  backproject, backprojection_cov                              :371-399
//  quadratic_fit                                                :401-491
//  the per-feature assembly of on_rgbd                          :547-634
//  mu_app, has_mu_app and the non-finite covariance             backend/backend_node.py:1600-1601, :1616-1620
//
// One kernel, f64, one wavefront per keypoint and one lane per window pixel (the windows hold at most
// 7 x 7 = 49 pixels), no atomics and no LDS: every value of a keypoint is the same on all 64 lanes, lane
// 0 stores it, and the outputs are bitwise the same from run to run.
//
//  the depth window   lane l holds pixel l of the window in row-major order (the order the node pushes
//                     zs in) or hex offset l; a pixel outside the image or without a finite positive
//                     depth takes no part (the ballot is the node's zs).
//  median, MAD        the element of rank size/2 (std::nth_element at zs.begin() + zs.size() / 2) by rank
//                     counting across lanes: a lane's rank is the number of valid lanes whose value is
//                     smaller, or equal with a lower lane index; the lane of that rank hands its value out.
//  sums               the mean, the variance, the Student-t residual sum and the 21 + 6 normal-equation
//                     sums by the wave butterfly of gc_blocksum.h (group_sum_xor<64>). The node adds in
//                     zs order after nth_element has permuted it, which is unspecified.
//  the fit            AᵀA + εI by an unpivoted LDLᵀ in registers, fully unrolled (Eigen's ldlt() pivots on
//                     the diagonal; the two agree to rounding times cond(AᵀA + εI)), the smaller eigenvalue
//                     of the symmetric 2 x 2 H_uv in closed form (Eigen iterates).
//
// The hex offsets round(r cos(k π/3)), round(r sin(k π/3)) are computed on the host as the node computes
// them and travel in the kernel arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"

// no fused multiply-adds anywhere in this file, the inlined helpers included (as k_cs_finish)
#pragma clang fp contract(off)

namespace gc {
namespace {

constexpr int kCfWave = 64;
constexpr int kCfMaxRadius = GC_CAMFEAT_MAX_RADIUS;  // (2 r + 1)^2 <= 49 lanes
constexpr int kCfHex = 7;        // the centre and six neighbours
constexpr int64_t kCfMaxQueries = GC_CAM_MAX_QUERIES;
constexpr int64_t kCfMaxPixels = GC_IMAGE_MAX_PIXELS;
constexpr double kCfEps = 1e-12;  // kEps (:34)
static_assert((2 * kCfMaxRadius + 1) * (2 * kCfMaxRadius + 1) <= kCfWave, "one lane per window pixel");

enum { kCfNearest = 0, kCfMedian3 = 1, kCfMedian5 = 2, kCfHexMode = 3 };

struct CfArgs {
  int H, W, mode, model, rq, min_points;
  int hx[kCfHex], hy[kCfHex];
  double fx, fy, cx, cy;
  double pixel_var, sigma0, sigma_slope, min_depth, max_depth, validity_slope, response_scale, depth_scale,
      invalid_cov, ridge, nu, w_min, ma_tau, ma_delta, kappa0, kappa_alpha, kappa_max, kappa_min;
  const float* depth;
  const uint8_t* rgb;
  const double* kp;
  double *uv, *Lc, *thc, *weight, *kappa, *mu, *color, *xyz, *cov, *aux;
  uint8_t *has_mu, *has_color;
};

GC_DEV double cf_max(double a, double b) { return a < b ? b : a; }  // std::max(a, b)
GC_DEV double cf_min(double a, double b) { return b < a ? b : a; }  // std::min(a, b)
GC_DEV double cf_clamp(double v, double lo, double hi) { return cf_max(lo, cf_min(hi, v)); }  // :46-49
GC_DEV bool cf_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }             // false for NaN

// lane l of a side x side window of radius r: its row and column offsets
GC_DEV void cf_window_offset(int l, int r, int* dx, int* dy) {
  const int row = r == 1 ? l / 3 : (r == 2 ? l / 5 : (r == 3 ? l / 7 : l));
  *dy = row - r;
  *dx = l - row * (2 * r + 1) - r;
}

// depth_to_meters of pixel (xi, yi) and whether the node keeps it (:268-271, :319-322, :414-418)
GC_DEV bool cf_depth_at(const CfArgs& a, bool want, int xi, int yi, double* z) {
  *z = 0.0;
  if (!(want && xi >= 0 && xi < a.W && yi >= 0 && yi < a.H)) return false;
  *z = (double)a.depth[(int64_t)yi * a.W + xi] * a.depth_scale;
  return cf_finite(*z) && *z > 0.0;
}

// the value of rank k (from 0) among the lanes set in vm, ties to the lower lane; nl: lanes in use.
// All 64 lanes call it together. With k past the count the result is lane 0's value and unused.
GC_DEV double cf_rank_select(double x, unsigned long long vm, int nl, int k) {
  const int lane = threadIdx.x;
  int rank = 0;
  for (int j = 0; j < nl; ++j) {
    const double xj = __shfl(x, j, kCfWave);
    const bool before = xj < x || (xj == x && j < lane);
    rank += (((vm >> j) & 1ull) && before) ? 1 : 0;
  }
  const unsigned long long hit = __ballot(((vm >> lane) & 1ull) && rank == k);
  return __shfl(x, hit ? __ffsll((long long)hit) - 1 : 0, kCfWave);
}

GC_DEV double cf_depth_sigma(const CfArgs& a, double z_m) {  // :216-226
  const double z = fabs(z_m);
  return a.model == 0 ? a.sigma0 + a.sigma_slope * z : a.sigma0 + a.sigma_slope * (z * z);
}

__global__ void __launch_bounds__(kCfWave) k_cf_lift(CfArgs a) {
  const int lane = threadIdx.x;
  const int64_t m = blockIdx.x;
  const double nan = __builtin_nan("");
  const double u = a.kp[3 * m], v = a.kp[3 * m + 1], response = a.kp[3 * m + 2];
  // ---- depth_sample (:228-297): std::round rounds half away from zero, as round() does
  const double ru = round(u), rv = round(v);
  const bool in_img = ru >= 0.0 && rv >= 0.0 && ru < (double)a.W && rv < (double)a.H;  // false for NaN
  const int x = in_img ? (int)ru : 0, y = in_img ? (int)rv : 0;
  int nl = 1, dx = 0, dy = 0;
  if (a.mode == kCfMedian3 || a.mode == kCfMedian5) {
    const int r = a.mode == kCfMedian3 ? 1 : 2;
    nl = (2 * r + 1) * (2 * r + 1);
    cf_window_offset(lane, r, &dx, &dy);
  } else if (a.mode == kCfHexMode) {
    nl = kCfHex;
#pragma unroll
    for (int q = 0; q < kCfHex; ++q)
      if (lane == q) { dx = a.hx[q]; dy = a.hy[q]; }
  }
  double z;
  const bool valid = cf_depth_at(a, in_img && lane < nl, x + dx, y + dy, &z);
  const unsigned long long vm = __ballot(valid);
  const int n_win = __popcll(vm);
  bool z_valid = false;
  double z_m = nan, z_var = nan;
  if (a.mode == kCfNearest) {
    z_valid = n_win == 1;
    if (z_valid) z_m = __shfl(z, 0, kCfWave);
  } else if (a.mode == kCfHexMode) {
    if (n_win >= 4) {  // :327
      z_m = cf_rank_select(z, vm, nl, n_win / 2);
      const double mad = cf_rank_select(fabs(z - z_m), vm, nl, n_win / 2);
      const double sigma_z = 1.4826 * mad;
      z_var = sigma_z * sigma_z;
      z_valid = true;
    }
  } else if (n_win >= 1) {
    z_m = cf_rank_select(z, vm, nl, n_win / 2);
    z_valid = true;
    if (n_win >= 4) {  // :282-292
      const double mean = group_sum_xor<kCfWave>(valid ? z : 0.0) / (double)n_win;
      const double d = z - mean;
      z_var = group_sum_xor<kCfWave>(valid ? d * d : 0.0) / (double)n_win;
    }
  }
  if (!cf_finite(z_var)) z_var = nan;  // validate_depth (:191)
  // ---- the weight (:554-556)
  double w_depth = 0.0;
  if (z_valid) {  // depth_weight (:196-205); z_m is finite
    const double w_lo = 1.0 / (1.0 + exp(-a.validity_slope * (z_m - a.min_depth)));
    const double w_hi = 1.0 / (1.0 + exp(+a.validity_slope * (z_m - a.max_depth)));
    w_depth = cf_clamp(w_lo * w_hi, 0.0, 1.0);
  }
  const double w_resp = response <= 0.0 ? 0.0 : response / (response + a.response_scale);  // :207-214
  const double weight = cf_clamp(w_depth * w_resp, 0.0, 1.0);
  // ---- var_z_eff (:563-572) with student_t_effective_var (:350-369)
  const double sig = z_valid ? cf_depth_sigma(a, z_m) : 0.0, sig_sq = sig * sig;
  double var_z_eff = nan;
  if (z_valid && cf_finite(z_var)) {
    const double base_var = cf_max(z_var, sig_sq);
    var_z_eff = base_var;
    if (!(n_win < 2 || !cf_finite(base_var) || base_var <= 0.0)) {
      const double sigma2 = cf_max(base_var, kCfEps);
      const double res = z - z_m;
      double q = group_sum_xor<kCfWave>(valid ? res * res : 0.0);
      q /= ((double)n_win * sigma2 + kCfEps);
      double w = (a.nu + 1.0) / (a.nu + q);
      if (w < a.w_min) w = a.w_min;
      var_z_eff = base_var / w;
    }
  } else if (z_valid) {
    var_z_eff = sig_sq;
  }
  if (z_valid && !cf_finite(var_z_eff)) var_z_eff = sig_sq;
  // ---- quadratic_fit (:401-491)
  bool fit = false;
  int n_fit = 0;
  double normal[3] = {0.0, 0.0, 0.0}, K = 0.0, lam_min = 0.0;
  if (z_valid) {
    int qx, qy;
    cf_window_offset(lane, a.rq, &qx, &qy);
    const int xi = x + qx, yi = y + qy;
    double zi;
    const bool vq = cf_depth_at(a, lane < (2 * a.rq + 1) * (2 * a.rq + 1), xi, yi, &zi);
    n_fit = __popcll(__ballot(vq));
    if (n_fit >= a.min_points) {
      const double u_t = (double)xi - u, v_t = (double)yi - v;
      const double row[6] = {u_t * u_t, u_t * v_t, v_t * v_t, u_t, v_t, 1.0};
      // AᵀA (lower triangle) and Aᵀb: every lane ends with the same sums
      double A[6][6], b[6];
#pragma unroll
      for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int q = 0; q <= p; ++q) A[p][q] = group_sum_xor<kCfWave>(vq ? row[p] * row[q] : 0.0);
        b[p] = group_sum_xor<kCfWave>(vq ? row[p] * zi : 0.0);
      }
#pragma unroll
      for (int p = 0; p < 6; ++p) A[p][p] += a.ridge;  // :443
      // A = L D Lᵀ, unit lower L, no pivoting; then L y = b, D w = y, Lᵀ beta = w
      double L[6][6], D[6], beta[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
          double s = A[i][j];
#pragma unroll
          for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * D[k];
          L[i][j] = s / d;
        }
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * beta[k];
        beta[i] = s;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) beta[i] = beta[i] / D[i];
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double s = beta[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * beta[k];
        beta[i] = s;
      }
      // :447-481
      const double zc = cf_max(z_m, 1e-6);
      const double sx = a.fx / zc, sy = a.fy / zc;
      const double zu = sx * beta[3], zv = sy * beta[4];
      const double h00 = sx * sx * (2.0 * beta[0]), h01 = sx * sy * beta[1], h11 = sy * sy * (2.0 * beta[2]);
      const double det_H = h00 * h11 - h01 * h01;
      const double denom = 1.0 + (zu * zu + zv * zv);
      K = denom > 0.0 ? det_H / (denom * denom) : 0.0;
      const double hm = 0.5 * (h00 + h11), hd = 0.5 * (h00 - h11);
      lam_min = hm - sqrt(hd * hd + h01 * h01);
      normal[0] = -zu; normal[1] = -zv; normal[2] = 1.0;
      const double nn = sqrt(zu * zu + zv * zv + 1.0);
      if (nn > 0.0) { normal[0] /= nn; normal[1] /= nn; normal[2] /= nn; }
      fit = true;
    }
  }
  if (lane != 0) return;
  // ---- the assembly (:574-634)
  double xyz[3] = {0.0, 0.0, 0.0};
  double cov[9] = {a.invalid_cov, 0.0, 0.0, 0.0, a.invalid_cov, 0.0, 0.0, 0.0, a.invalid_cov};
  const double w_ma = fit ? sigmoid(a.ma_tau * lam_min) : 0.0;
  if (z_valid) {
    const double du = u - a.cx, dv = v - a.cy;
    xyz[0] = du * z_m / a.fx;  // :373-375
    xyz[1] = dv * z_m / a.fy;
    xyz[2] = z_m;
    const double vu = cf_max(a.pixel_var, 0.0), vv = vu, vz = cf_max(cf_max(var_z_eff, sig_sq), 0.0);  // :579, :382-384
    const double var_x = (z_m * z_m * vu + du * du * vz + vu * vz) / (a.fx * a.fx);
    const double var_y = (z_m * z_m * vv + dv * dv * vz + vv * vz) / (a.fy * a.fy);
    const double cxy = (du * dv * vz) / (a.fx * a.fy), cxz = (du * vz) / a.fx, cyz = (dv * vz) / a.fy;
    cov[0] = var_x; cov[1] = cxy; cov[2] = cxz;
    cov[3] = cxy; cov[4] = var_y; cov[5] = cyz;
    cov[6] = cxz; cov[7] = cyz; cov[8] = vz;
    if (fit) {  // :581-584
      const double inflate = (1.0 - w_ma) * a.ma_delta;
      cov[0] += inflate; cov[4] += inflate; cov[8] += inflate;
    }
  }
  double kappa_app = 0.0;
  if (fit) {  // :589-600
    const double rel_noise = (z_valid && cf_finite(var_z_eff)) ? sqrt(var_z_eff) / (z_m + kCfEps) : 1.0;
    const double rho = 1.0 / (rel_noise + kCfEps);
    kappa_app = a.kappa0 + a.kappa_alpha * sqrt(fabs(K)) * rho;
    kappa_app = cf_clamp(kappa_app, a.kappa_min, a.kappa_max);
    kappa_app = kappa_app * w_ma;
  }
  double sigma_c_sq = nan, Lambda_c = 0.0, theta_c = 0.0;
  if (z_valid && cf_finite(var_z_eff) && var_z_eff > 0.0) {  // :605-609
    sigma_c_sq = var_z_eff;
    Lambda_c = 1.0 / sigma_c_sq;
    theta_c = Lambda_c * z_m;
  }
  // backend_node.py:1600-1601: a covariance with a non-finite entry becomes 1e6 I
  bool cov_finite = true;
#pragma unroll
  for (int q = 0; q < 9; ++q) cov_finite = cov_finite && cf_finite(cov[q]);
  // backend_node.py:1616-1620
  const double mu_norm = sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
  const bool has_mu = fit && cf_finite(normal[0]) && cf_finite(normal[1]) && cf_finite(normal[2]) && mu_norm > 0.0;
  a.uv[2 * m] = u;
  a.uv[2 * m + 1] = v;
  a.Lc[m] = Lambda_c;
  a.thc[m] = theta_c;
  a.weight[m] = weight;
  a.kappa[m] = kappa_app;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a.mu[3 * m + q] = has_mu ? normal[q] / (mu_norm + 1e-12) : 0.0;
    a.xyz[3 * m + q] = xyz[q];
  }
  a.has_mu[m] = has_mu ? 1 : 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) a.cov[9 * m + q] = cov_finite ? cov[q] : (q % 4 == 0 ? 1e6 : 0.0);
  // the colour at the clamped, rounded pixel, whether or not the depth is valid (:611-616)
  double rgb[3] = {0.0, 0.0, 0.0};
  if (a.rgb) {
    const int ix = (int)round(cf_clamp(u, 0.0, (double)(a.W - 1)));
    const int iy = (int)round(cf_clamp(v, 0.0, (double)(a.H - 1)));
    const uint8_t* px = a.rgb + 3 * ((int64_t)iy * a.W + ix);
#pragma unroll
    for (int q = 0; q < 3; ++q) rgb[q] = (double)px[q] / 255.0;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) a.color[3 * m + q] = rgb[q];
  a.has_color[m] = a.rgb ? 1 : 0;
  double* x6 = a.aux + GC_CAMFEAT_AUX * m;
  x6[0] = sigma_c_sq;
  x6[1] = z_m;
  x6[2] = (double)n_win;
  x6[3] = (double)n_fit;
  x6[4] = lam_min;
  x6[5] = K;
}

int cf_parse(gc_ctx* ctx, const double* k, const gc_camfeat_cfg* h, CfArgs* a) {
  for (int q = 0; q < 4; ++q) GC_CHECK_ARG(ctx, fabs(k[q]) <= 1e300, "the intrinsics must be finite");
  GC_CHECK_ARG(ctx, k[0] != 0.0 && k[1] != 0.0, "fx and fy must not be 0");
  GC_CHECK_ARG(ctx, cfg_all<24>(h, [](double v) { return v == v; }), "NaN in the configuration");
  const double mode = h->depth_sample_mode, rh = h->hex_radius, rq = h->quad_fit_radius, mp = h->quad_fit_min_points;
  GC_CHECK_ARG(ctx, mode == 0.0 || mode == 1.0 || mode == 2.0 || mode == 3.0,
               "depth_sample_mode must be 0 (nearest), 1 (median3), 2 (median5) or 3 (hex)");
  GC_CHECK_ARG(ctx, h->depth_model == 0.0 || h->depth_model == 1.0, "depth_model must be 0 (linear) or 1 (quadratic)");
  // std::max(1, r) first (:303, :407)
  GC_CHECK_ARG(ctx, rh == floor(rh) && rh <= (double)kCfMaxRadius && rh >= -2147483648.0,
               "hex_radius must be an integer with max(1, hex_radius) in [1, 3]");
  GC_CHECK_ARG(ctx, rq == floor(rq) && rq <= (double)kCfMaxRadius && rq >= -2147483648.0,
               "quad_fit_radius must be an integer with max(1, quad_fit_radius) in [1, 3]");
  GC_CHECK_ARG(ctx, mp == floor(mp) && mp >= 1.0 && mp <= 16777216.0, "quad_fit_min_points must be an integer >= 1");
  a->fx = k[0]; a->fy = k[1]; a->cx = k[2]; a->cy = k[3];
  a->mode = (int)mode; a->pixel_var = h->pixel_sigma * h->pixel_sigma; /* :580 */ a->model = (int)h->depth_model;
  a->sigma0 = h->depth_sigma0; a->sigma_slope = h->depth_sigma_slope; a->min_depth = h->min_depth_m;
  a->max_depth = h->max_depth_m; a->validity_slope = h->depth_validity_slope;
  a->response_scale = h->response_soft_scale; a->depth_scale = h->depth_scale;
  a->invalid_cov = h->invalid_cov_inflate;  // cov_reg_eps before it: the node never reads it
  const int r_hex = rh < 1.0 ? 1 : (int)rh; a->rq = rq < 1.0 ? 1 : (int)rq; a->min_points = (int)mp;
  a->ridge = h->quad_fit_lstsq_eps; a->nu = h->student_t_nu; a->w_min = h->student_t_w_min; a->ma_tau = h->ma_tau;
  a->ma_delta = h->ma_delta_inflate; a->kappa0 = h->kappa0; a->kappa_alpha = h->kappa_alpha;
  a->kappa_max = h->kappa_max; a->kappa_min = h->kappa_min;
  // :304-312
  a->hx[0] = 0; a->hy[0] = 0;
  for (int q = 0; q < 6; ++q) {
    const double ang = (double)q * M_PI / 3.0;
    a->hx[q + 1] = (int)round(r_hex * cos(ang));
    a->hy[q + 1] = (int)round(r_hex * sin(ang));
  }
  return GC_OK;
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_camera_features_lift(gc_ctx* ctx, int32_t H, int32_t W, const float* d_depth, const uint8_t* d_rgb,
                                int64_t M, const double* d_kp, const double* h_intrinsics, const gc_camfeat_cfg* cfg,
                                double* d_uv, double* d_Lambda_c, double* d_theta_c, double* d_weight,
                                double* d_kappa, double* d_mu_app, uint8_t* d_has_mu_app, double* d_color,
                                uint8_t* d_has_color, double* d_xyz, double* d_cov_xyz, double* d_aux) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, h_intrinsics && cfg, "NULL argument");
  GC_CHECK_ARG(ctx, M >= 0 && M <= kCfMaxQueries, "M must be in [0, 4096]");
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && (int64_t)H * W <= kCfMaxPixels, "H and W must be >= 1 and H W <= 2^26");
  GC_CHECK_ARG(ctx, d_depth != nullptr, "NULL depth image");
  GC_CHECK_ARG(ctx, M == 0 || (d_kp && d_uv && d_Lambda_c && d_theta_c && d_weight && d_kappa && d_mu_app &&
                               d_has_mu_app && d_color && d_has_color && d_xyz && d_cov_xyz && d_aux),
               "NULL keypoint or output buffer");
  CfArgs a = {};
  if (int rc = cf_parse(ctx, h_intrinsics, cfg, &a)) return rc;
  if (M == 0) return GC_OK;
  a.H = H; a.W = W; a.depth = d_depth; a.rgb = d_rgb; a.kp = d_kp;
  a.uv = d_uv; a.Lc = d_Lambda_c; a.thc = d_theta_c; a.weight = d_weight; a.kappa = d_kappa; a.mu = d_mu_app;
  a.has_mu = d_has_mu_app; a.color = d_color; a.has_color = d_has_color; a.xyz = d_xyz; a.cov = d_cov_xyz;
  a.aux = d_aux;
  hipLaunchKernelGGL(k_cf_lift, dim3((unsigned)M), dim3(kCfWave), 0, ctx->stream, a);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
