// gc_depthev.hip — depth pose evidence from the camera view ("Depth pose evidence"): the
// depth image gc_render_depth_tiles composites, held against an observed depth frame and linearised in
// the body pose without a backward pass. A pose has six degrees of freedom, so every pixel carries the
// six tangents of its (T, D) forward through the compositing loop.
//
//   gc_camera_splat_jvp     per (pose, primitive): the six tangents of gc_camera_splat_prep's pixel mean,
//                           depth and inverse pixel covariance, from the same cam_project (gc_renderdev.h).
//   gc_depth_pose_evidence  per (pose, tile): the tile's list staged through LDS in chunks of kEvChunk
//                           records, one thread per pixel with (T, D, dT[6], dD[6]) in registers, stepped
//                           by the camera raster's cam_step_alpha / cam_step_through (gc_renderdev.h), then
//                           J, r, w per pixel and one fixed-order workgroup sum of the 31 values; per pose:
//                           the tiles in tile order, and L_pose / h_pose / parts filled or accumulated.
//
// The tangent convention is visual_pose_evidence.py's (r = map - (R m + t), d/dt = -I, :89-99;
// R_delta = R_scatter R_pred^T, :234-238): t_wb' = t_wb + dt, R_wb' = Exp(dtheta) R_wb. No floating-point
// atomics: the outputs are bitwise reproducible from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_renderdev.h"

namespace gc {
namespace {

constexpr int kEvMaxTile = 16;  // a thread owns one pixel
constexpr int kEvRec = 44;      // a record: mean 2, Sigma^-1 4, alpha, depth, dmean 12, ddepth 6, dSigma^-1 18
constexpr int kEvChunk = 64;    // records staged per barrier pair: 22 KB of LDS
constexpr int kEvNV = GC_DEPTHEV_PARTIAL;
constexpr int kEvParts = GC_DEPTHEV_PARTS;
static_assert(kEvNV == 21 + 6 + 4 && kEvParts == 36 + 6 + 4, "gcslam.h");
static_assert(kEvMaxTile * kEvMaxTile == kRdT, "one thread per pixel of the largest tile");
static_assert(kRdT % 4 == 0 && kEvRec % 4 == 0 && kEvChunk * 4 == kRdT, "four threads stage one record");

// ------------------------------------------------------------------------------------------------
// tangent prep
// ------------------------------------------------------------------------------------------------

// poses v0 .. v0 + n_views - 1, one lane per (pose, primitive); the forward quantities are cam_project's, as
// in k_cam_prep, the inverse pixel covariance and the validity are read from that kernel's outputs
__global__ __launch_bounds__(kRdT) void k_ev_jvp(int64_t n, int v0, int n_views, gc_render_batch b, CamViews views,
                                                 const double* Sinv, const uint8_t* valid, double* dmeans,
                                                 double* ddepths, double* dSinv) {
  const int64_t gl = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (gl >= n * n_views) return;
  const int vl = (int)(gl / n);
  const int64_t i = gl - (int64_t)vl * n;
  const int64_t g = (int64_t)(v0 + vl) * n + i;
  double* om = dmeans + 12 * g;
  double* od = ddepths + 6 * g;
  double* os = dSinv + 18 * g;
  if (!valid[g]) {
#pragma unroll
    for (int q = 0; q < 12; ++q) om[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) od[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 18; ++q) os[q] = 0.0;
    return;
  }
  const double* V = views.v + kCamView * vl;
  double R[9], S[9], mu[3], rel[3];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    R[q] = V[kCvR + q];
    S[q] = b.Sigma_world[9 * i + q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    mu[q] = b.mu_world[3 * i + q];
    rel[q] = mu[q] - V[kCvTwb + q];
  }
  CamProj P;
  cam_project(V, mu, S, P);
  const double *M = P.M, *MS = P.MS;
  const double fx = V[kCvFx], fy = V[kCvFy], limx = V[kCvLimX], limy = V[kCvLimY];
  const double x = P.p[0], y = P.p[1], z = P.p[2];
  const double ux = P.ux, uy = P.uy, tx = P.tx, ty = P.ty;
  // dtx = cx_d dx + cx_z dz: (1, 0) where the tangent is free, (0, +-lim) where it is clamped
  const double cxd = (ux < -limx || ux > limx) ? 0.0 : 1.0, cxz = ux < -limx ? -limx : (ux > limx ? limx : 0.0);
  const double cyd = (uy < -limy || uy > limy) ? 0.0 : 1.0, cyz = uy < -limy ? -limy : (uy > limy ? limy : 0.0);
  const double iz = 1.0 / z, iz2 = iz * iz, iz3 = iz2 * iz;
  const double J00 = P.J00, J02 = P.J02, J11 = P.J11, J12 = P.J12;
  double SMt[6];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      SMt[3 * r + k] = S[3 * k] * M[3 * r] + S[3 * k + 1] * M[3 * r + 1] + S[3 * k + 2] * M[3 * r + 2];  // (S M^T)[k][r]
  const double i00 = Sinv[4 * g], i01 = Sinv[4 * g + 1], i11 = Sinv[4 * g + 3];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double dp[3], dR[9];
    if (k < 3) {
#pragma unroll
      for (int r = 0; r < 3; ++r) dp[r] = -R[3 * r + k];
#pragma unroll
      for (int q = 0; q < 9; ++q) dR[q] = 0.0;
    } else {
      const int a = k - 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
      // (mu - t_wb) x e_a: component a1 is rel[a2], component a2 is -rel[a1]
      double c[3];
      c[a] = 0.0;
      c[a1] = rel[a2];
      c[a2] = -rel[a1];
#pragma unroll
      for (int r = 0; r < 3; ++r) dp[r] = R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2];
      // -R [e_a]x: [e_a]x has -1 at (a1, a2) and +1 at (a2, a1)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        dR[3 * r + a] = 0.0;
        dR[3 * r + a2] = R[3 * r + a1];
        dR[3 * r + a1] = -R[3 * r + a2];
      }
    }
    const double dx = dp[0], dy = dp[1], dz = dp[2];
    om[2 * k] = fx * (dx * iz - x * dz * iz2);
    om[2 * k + 1] = fy * (dy * iz - y * dz * iz2);
    od[k] = dz;
    const double dtx = cxd * dx + cxz * dz, dty = cyd * dy + cyz * dz;
    const double dJ00 = -fx * dz * iz2, dJ02 = -fx * (dtx * iz2 - 2.0 * tx * dz * iz3);
    const double dJ11 = -fy * dz * iz2, dJ12 = -fy * (dty * iz2 - 2.0 * ty * dz * iz3);
    double dM[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dM[c] = dJ00 * R[c] + dJ02 * R[6 + c] + J00 * dR[c] + J02 * dR[6 + c];
      dM[3 + c] = dJ11 * R[3 + c] + dJ12 * R[6 + c] + J11 * dR[3 + c] + J12 * dR[6 + c];
    }
    // dSp = dM (S M^T) + (M S) dM^T
    double dSp[4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        dSp[2 * r + c] = dM[3 * r] * SMt[3 * c] + dM[3 * r + 1] * SMt[3 * c + 1] + dM[3 * r + 2] * SMt[3 * c + 2] +
                         MS[3 * r] * dM[3 * c] + MS[3 * r + 1] * dM[3 * c + 1] + MS[3 * r + 2] * dM[3 * c + 2];
    const double da = dSp[0], dd = dSp[3], db = 0.5 * (dSp[1] + dSp[2]);
    const double t00 = i00 * da + i01 * db, t01 = i00 * db + i01 * dd;
    const double t10 = i01 * da + i11 * db, t11 = i01 * db + i11 * dd;
    os[3 * k] = -(t00 * i00 + t01 * i01);
    os[3 * k + 1] = -(t00 * i01 + t01 * i11);
    os[3 * k + 2] = -(t10 * i01 + t11 * i11);
  }
}

// ------------------------------------------------------------------------------------------------
// the evidence raster
// ------------------------------------------------------------------------------------------------

// the part of the camera view's configuration the evidence reads (from a checked CamCfg), then its own
struct EvCfg {
  double alpha_max, alpha_skip, t_stop, eps;
  double sigma0, slope, dmin, dmax, nu;
  int quadratic, robust;
};

struct EvRasterArgs {
  int64_t n;
  TileGrid G;
  int H, W, cap;
  const double *means, *Sinv, *alphas, *depths, *dmeans, *ddepths, *dSinv;
  const int32_t *indices, *counts;
  const double *alpha_img, *depth_img;
  const float* obs;
  EvCfg c;
  double *partial, *residual, *weight;
};

// One workgroup per (pose, tile), thread p the pixel p of the row-major tile (p < ts^2 <= 256). The list is
// staged kEvChunk records at a time (four threads per record), a barrier on either side; every lane reads
// the same record per step. A wave whose pixels have all stopped skips the arithmetic but keeps the
// barriers; the workgroup leaves the list once every pixel has stopped.
__global__ __launch_bounds__(kRdT) void k_ev_raster(EvRasterArgs A) {
  __shared__ double rec[kEvChunk * kEvRec];
  __shared__ double red[(kRdT / 64) * kEvNV];
  const int64_t seg = blockIdx.x;
  const int ts = A.G.ts;
  int ox, oy;  // the image's: the grid's origin is 0 (rd_tile_grid)
  const int64_t v = rd_seg_tile(seg, A.G, ox, oy);
  const int m = rd_clamp_count(A.counts[seg], A.cap);
  const int p = threadIdx.x;
  const bool own = p < ts * ts;
  const int col = ox + (own ? p % ts : 0), row = oy + (own ? p / ts : 0);
  const double px = (double)col + 0.5, py = (double)row + 0.5;
  double Tr = 1.0, D = 0.0, dT[6], dD[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) dT[k] = dD[k] = 0.0;
  bool live = own;
  for (int c0 = 0; c0 < m; c0 += kEvChunk) {
    const int mc = m - c0 < kEvChunk ? m - c0 : kEvChunk;
    if (c0 > 0 && !__syncthreads_or(live ? 1 : 0)) break;  // also the barrier before rec is overwritten
    {
      const int e = threadIdx.x >> 2, part = threadIdx.x & 3;
      if (e < mc) {
        const int64_t i = rd_list_index(A.indices[seg * A.cap + c0 + e], A.n);
        const int64_t r = v * A.n + i;
        double* o = rec + kEvRec * e;
        if (part == 0) {
          o[0] = A.means[2 * r];
          o[1] = A.means[2 * r + 1];
#pragma unroll
          for (int q = 0; q < 4; ++q) o[2 + q] = A.Sinv[4 * r + q];
          o[6] = A.alphas[i];
          o[7] = A.depths[r];
        } else if (part == 1) {
#pragma unroll
          for (int q = 0; q < 12; ++q) o[8 + q] = A.dmeans[12 * r + q];
        } else if (part == 2) {
#pragma unroll
          for (int q = 0; q < 6; ++q) o[20 + q] = A.ddepths[6 * r + q];
#pragma unroll
          for (int q = 0; q < 6; ++q) o[26 + q] = A.dSinv[18 * r + q];
        } else {
#pragma unroll
          for (int q = 6; q < 18; ++q) o[26 + q] = A.dSinv[18 * r + q];
        }
      }
    }
    __syncthreads();
    for (int j = 0; j < mc; ++j) {
      if (!__any(live)) break;  // wave-uniform; the barriers are outside this loop
      const double* o = rec + kEvRec * j;
      const double mx = o[0], my = o[1], s00 = o[2], s01 = o[3], s10 = o[4], s11 = o[5], al = o[6], dep = o[7];
      const double d0 = px - mx, d1 = py - my;
      const double q = rd_quad(d0, d1, s00, s01, s10, s11);
      double raw, a;
      cam_step_alpha(al, q, A.c.alpha_max, raw, a);
      if (live && a >= A.c.alpha_skip) {
        const bool flat = raw > A.c.alpha_max || q < 0.0;
        const double g0 = s00 * d0 + s01 * d1, g1 = s10 * d0 + s11 * d1;
        const double d00 = d0 * d0, d01 = 2.0 * d0 * d1, d11 = d1 * d1;
        const double Ta = Tr * a, az = a * dep, Tz = Tr * dep, na = 1.0 - a;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double dq = -2.0 * (g0 * o[8 + 2 * k] + g1 * o[9 + 2 * k]) +
                            (o[26 + 3 * k] * d00 + o[27 + 3 * k] * d01 + o[28 + 3 * k] * d11);
          const double da = flat ? 0.0 : -0.5 * a * dq;
          dD[k] += dT[k] * az + Tz * da + Ta * o[20 + k];
          dT[k] = dT[k] * na - Tr * da;
        }
        D += Ta * dep;
        if (cam_step_through(Tr, a, A.c.t_stop)) live = false;
      }
    }
  }
  // the pixel's evidence
  double val[kEvNV];
#pragma unroll
  for (int q = 0; q < kEvNV; ++q) val[q] = 0.0;
  double r_out = 0.0, w_out = 0.0;
  const int64_t at = (v * A.H + row) * A.W + col;
  if (own) {
    const double cover = A.alpha_img[at];
    const double obs = (double)A.obs[(int64_t)row * A.W + col];
    const bool used = fabs(obs) < HUGE_VAL && obs > A.c.dmin && obs < A.c.dmax && cover > A.c.eps;
    if (used) {
      const double r = A.depth_img[at] - obs;
      const double sg = A.c.sigma0 + A.c.slope * (A.c.quadratic ? obs * obs : obs);
      const double rs = r / sg;
      const double u = A.c.robust ? (A.c.nu + 1.0) / (A.c.nu + rs * rs) : 1.0;
      const double w = cover * u / (sg * sg);
      const double ia2 = 1.0 / (cover * cover);
      double J[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) J[k] = (dD[k] * cover + D * dT[k]) * ia2;
      int e = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double wj = w * J[i];
#pragma unroll
        for (int j = i; j < 6; ++j) val[e++] = wj * J[j];
        val[21 + i] = wj * r;
      }
      val[27] = w * r * r;
      val[28] = 1.0;
      val[29] = cover;
      val[30] = w;
      r_out = r;
      w_out = w;
    }
    if (A.residual) A.residual[at] = r_out;
    if (A.weight) A.weight[at] = w_out;
  }
  __syncthreads();
  block_sum<kEvNV, kRdT / 64>(val, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kEvNV; ++q) A.partial[seg * kEvNV + q] = val[q];
  }
}

// one workgroup per pose: the tiles in a fixed order, then L_pose, h_pose and the parts row
__global__ __launch_bounds__(kRdT) void k_ev_final(int G, const double* partial, double eps_lift, int accumulate,
                                                   double* L_pose, double* h_pose, double* parts) {
  __shared__ double stage[kRdT], tot[32];
  const int v = blockIdx.x;
  sum_partials<32, kRdT>(G, partial + (int64_t)v * G * kEvNV, kEvNV, stage, tot);
  double* L = L_pose + (int64_t)v * 484;
  double* h = h_pose + (int64_t)v * 22;
  double* P = parts + (int64_t)v * kEvParts;
  const int tid = threadIdx.x;
  if (!accumulate) {
    for (int e = tid; e < 484; e += kRdT) {
      const int r = e / 22, c = e % 22;
      if (r >= 6 || c >= 6) L[e] = 0.0;
    }
    if (tid >= 6 && tid < 22) h[tid] = 0.0;
  }
  if (tid < 36) {
    const int r = tid / 6, c = tid % 6;
    const int i = r < c ? r : c, j = r < c ? c : r;
    const double x = tot[i * 6 - (i * (i - 1)) / 2 + (j - i)];  // row i of the upper triangle starts at 6 i - i (i - 1) / 2
    P[tid] = x;
    if (accumulate) L[r * 22 + c] += x;
    else L[r * 22 + c] = x + (r == c ? eps_lift : 0.0);
  } else if (tid < 42) {
    const double x = -tot[21 + (tid - 36)];
    P[tid] = x;
    if (accumulate) h[tid - 36] += x;
    else h[tid - 36] = x;
  } else if (tid < kEvParts) {
    P[tid] = tot[27 + (tid - 42)];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_camera_splat_jvp(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_poses, const double* h_T_cw,
                            const double* h_t_wb, const double* h_intrinsics, int32_t H, int32_t W,
                            const gc_camview_cfg* cfg, const gc_cam_splats* splats, double* d_dmeans_px,
                            double* d_ddepths, double* d_dSigmas_inv) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, batch && h_T_cw && h_t_wb && h_intrinsics && cfg && splats, "NULL argument");
  GC_CHECK_ARG(ctx, n >= 0 && n <= ((int64_t)1 << 24), "n must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, n_poses >= 1 && n_poses <= kRdMaxViews, "n_poses must be in [1, 32]");
  CamCfg c;
  if (int rc = cam_cfg(ctx, cfg, &c)) return rc;
  double hv[kRdMaxViews * kCamView];
  if (int rc = cam_pack_views(ctx, n_poses, h_T_cw, h_intrinsics, h_t_wb, H, W, hv)) return rc;
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, batch->mu_world && batch->Sigma_world, "NULL batch field");
  GC_CHECK_ARG(ctx, splats->Sigmas_inv && splats->valid, "NULL splat field");
  GC_CHECK_ARG(ctx, d_dmeans_px && d_ddepths && d_dSigmas_inv, "NULL output buffer");
  hipStream_t st = ctx->stream;
  return cam_each_launch(ctx, n_poses, hv, [&](int v0, int nv, const CamViews& views) {
    hipLaunchKernelGGL(k_ev_jvp, dim3(rd_blocks(n * nv)), dim3(kRdT), 0, st, n, v0, nv, *batch, views,
                       (const double*)splats->Sigmas_inv, (const uint8_t*)splats->valid, d_dmeans_px, d_ddepths,
                       d_dSigmas_inv);
  });
}

int32_t gc_depth_pose_evidence(gc_ctx* ctx, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                               const double* d_dmeans_px, const double* d_ddepths, const double* d_dSigmas_inv,
                               int32_t H, int32_t W, int32_t tile_size, int32_t cap, const gc_camview_cfg* cfg,
                               const int32_t* d_tile_counts, const int32_t* d_tile_indices, const double* d_alpha,
                               const double* d_depth, const float* d_depth_obs, int32_t depth_model, double sigma0,
                               double slope, double min_depth, double max_depth, int32_t use_robust, double robust_nu,
                               double eps_lift, int32_t accumulate, double* d_L_pose, double* d_h_pose,
                               double* d_parts, double* d_residual, double* d_weight) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  TileGrid G;
  int64_t segs;
  if (int rc = rd_tile_grid(ctx, n_poses, n, H, W, tile_size, kEvMaxTile, cap,
                            {"n_poses must be in [1, 32]", "tile_size must be in [1, 16]: a thread owns one pixel",
                             "H and W must be in [1, 16384]", "H and W must be multiples of tile_size",
                             "n_poses * tiles * n must be below 2^32"},
                            &G, &segs))
    return rc;
  CamCfg vc;
  if (int rc = cam_cfg(ctx, cfg, &vc)) return rc;
  EvRasterArgs A;
  A.c.alpha_max = vc.alpha_max; A.c.alpha_skip = vc.alpha_skip; A.c.t_stop = vc.t_stop; A.c.eps = vc.eps;
  GC_CHECK_ARG(ctx, depth_model == 0 || depth_model == 1, "depth_model must be 0 (linear) or 1 (quadratic)");
  GC_CHECK_ARG(ctx, rd_finite(sigma0) && rd_finite(slope) && rd_finite(min_depth) && rd_finite(max_depth) &&
                        rd_finite(eps_lift) && (!use_robust || rd_finite(robust_nu)),
               "the evidence parameters must be finite");
  GC_CHECK_ARG(ctx, sigma0 > 0.0 && slope >= 0.0, "depth_sigma0 must be > 0 and depth_sigma_slope >= 0");
  GC_CHECK_ARG(ctx, min_depth >= 0.0 && max_depth > min_depth, "the depth limits must satisfy 0 <= min < max");
  GC_CHECK_ARG(ctx, !use_robust || robust_nu > 0.0, "robust_nu must be > 0");
  GC_CHECK_ARG(ctx, eps_lift >= 0.0, "eps_lift must be >= 0");
  GC_CHECK_ARG(ctx, d_L_pose && d_h_pose && d_parts, "NULL output buffer");
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)n_poses * H * W;
  if (n == 0) {  // no raster over an empty range: the sums over no tile
    if (d_residual) GC_HIP(ctx, hipMemsetAsync(d_residual, 0, sizeof(double) * px, st));
    if (d_weight) GC_HIP(ctx, hipMemsetAsync(d_weight, 0, sizeof(double) * px, st));
    hipLaunchKernelGGL(k_ev_final, dim3((unsigned)n_poses), dim3(kRdT), 0, st, 0, (const double*)nullptr, eps_lift,
                       (int)(accumulate != 0), d_L_pose, d_h_pose, d_parts);
    GC_LAUNCH_CHECK(ctx);
    return GC_OK;
  }
  GC_CHECK_ARG(ctx, splats && splats->means_px && splats->Sigmas_inv && splats->depths && splats->alphas, "NULL splat field");
  GC_CHECK_ARG(ctx, d_dmeans_px && d_ddepths && d_dSigmas_inv, "NULL tangent array");
  GC_CHECK_ARG(ctx, d_tile_counts && d_tile_indices && d_alpha && d_depth && d_depth_obs, "NULL input buffer");
  double* partial;
  if (int rc = carve_scratch(ctx, [&](Carver& cv) { partial = cv.take<double>((size_t)segs * kEvNV); })) return rc;
  A.c.sigma0 = sigma0; A.c.slope = slope; A.c.dmin = min_depth; A.c.dmax = max_depth;
  A.c.nu = use_robust ? robust_nu : 0.0;
  A.c.quadratic = depth_model; A.c.robust = use_robust != 0;
  A.n = n; A.G = G; A.H = H; A.W = W; A.cap = cap;
  A.means = splats->means_px; A.Sinv = splats->Sigmas_inv; A.alphas = splats->alphas; A.depths = splats->depths;
  A.dmeans = d_dmeans_px; A.ddepths = d_ddepths; A.dSinv = d_dSigmas_inv;
  A.indices = d_tile_indices; A.counts = d_tile_counts;
  A.alpha_img = d_alpha; A.depth_img = d_depth; A.obs = d_depth_obs;
  A.partial = partial; A.residual = d_residual; A.weight = d_weight;
  hipLaunchKernelGGL(k_ev_raster, dim3((unsigned)segs), dim3(kRdT), 0, st, A);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_ev_final, dim3((unsigned)n_poses), dim3(kRdT), 0, st, (int)G.T, (const double*)partial, eps_lift,
                     (int)(accumulate != 0), d_L_pose, d_h_pose, d_parts);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
