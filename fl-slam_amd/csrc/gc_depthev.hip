// gc_depthev.hip — depth pose evidence from the camera view ("Depth pose evidence"): the
// depth image gc_render_depth_tiles composites, held against an observed depth frame and linearised in
// the body pose without a backward pass. A pose has six degrees of freedom, so every pixel carries the
// six tangents of its (T, D) forward through the compositing loop.
//
//   gc_camera_splat_jvp     per (pose, primitive): the six tangents of gc_camera_splat_prep's pixel mean,
//                           depth and inverse pixel covariance.
//   gc_depth_pose_evidence  per (pose, tile): the tile's list staged through LDS in chunks of kEvChunk
//                           records, one thread per pixel with (T, D, dT[6], dD[6]) in registers, then
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
constexpr int kEvView = 22;     // per pose: R (9), t (3), fx fy cx cy, t_wb (3), limx, limy, one pad
constexpr int kEvViewsPerLaunch = 16;
constexpr int kEvRec = 44;      // a record: mean 2, Sigma^-1 4, alpha, depth, dmean 12, ddepth 6, dSigma^-1 18
constexpr int kEvChunk = 64;    // records staged per barrier pair: 22 KB of LDS
constexpr int kEvNV = GC_DEPTHEV_PARTIAL;
constexpr int kEvParts = GC_DEPTHEV_PARTS;
static_assert(kEvNV == 21 + 6 + 4 && kEvParts == 36 + 6 + 4, "gcslam.h");
static_assert(kEvMaxTile * kEvMaxTile == kRdT, "one thread per pixel of the largest tile");
static_assert(kRdT % 4 == 0 && kEvRec % 4 == 0 && kEvChunk * 4 == kRdT, "four threads stage one record");

struct EvViews {
  double v[kEvViewsPerLaunch * kEvView];
};

// ------------------------------------------------------------------------------------------------
// tangent prep
// ------------------------------------------------------------------------------------------------

// poses v0 .. v0 + n_views - 1, one lane per (pose, primitive); the forward quantities are recomputed as
// k_cam_prep computes them, the inverse pixel covariance and the validity are read from its outputs
__global__ __launch_bounds__(kRdT) void k_ev_jvp(int64_t n, int v0, int n_views, gc_render_batch b, EvViews views,
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
  const double* V = views.v + kEvView * vl;
  double R[9], S[9], mu[3], p[3], rel[3];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    R[q] = V[q];
    S[q] = b.Sigma_world[9 * i + q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    mu[q] = b.mu_world[3 * i + q];
    rel[q] = mu[q] - V[16 + q];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = R[3 * r] * mu[0] + R[3 * r + 1] * mu[1] + R[3 * r + 2] * mu[2] + V[9 + r];
  const double fx = V[12], fy = V[13], limx = V[19], limy = V[20];
  const double x = p[0], y = p[1], z = p[2];
  const double ux = x / z, uy = y / z;
  const double tx = fmin(fmax(ux, -limx), limx) * z, ty = fmin(fmax(uy, -limy), limy) * z;
  // dtx = cx_d dx + cx_z dz: (1, 0) where the tangent is free, (0, +-lim) where it is clamped
  const double cxd = (ux < -limx || ux > limx) ? 0.0 : 1.0, cxz = ux < -limx ? -limx : (ux > limx ? limx : 0.0);
  const double cyd = (uy < -limy || uy > limy) ? 0.0 : 1.0, cyz = uy < -limy ? -limy : (uy > limy ? limy : 0.0);
  const double iz = 1.0 / z, iz2 = iz * iz, iz3 = iz2 * iz;
  const double J00 = fx / z, J02 = -fx * tx / (z * z), J11 = fy / z, J12 = -fy * ty / (z * z);
  double M[6], MS[6], SMt[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    M[k] = J00 * R[k] + J02 * R[6 + k];
    M[3 + k] = J11 * R[3 + k] + J12 * R[6 + k];
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      MS[3 * r + k] = M[3 * r] * S[k] + M[3 * r + 1] * S[3 + k] + M[3 * r + 2] * S[6 + k];       // (M S)[r][k]
      SMt[3 * r + k] = S[3 * k] * M[3 * r] + S[3 * k + 1] * M[3 * r + 1] + S[3 * k + 2] * M[3 * r + 2];  // (S M^T)[k][r]
    }
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
  const int64_t v = seg / A.G.T;
  const int t = (int)(seg - v * A.G.T);
  const int ts = A.G.ts;
  const int ox = (t % A.G.tiles_x) * ts, oy = (t / A.G.tiles_x) * ts;
  int m = A.counts[seg];
  m = m < 0 ? 0 : (m > A.cap ? A.cap : m);
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
        int64_t i = (int64_t)A.indices[seg * A.cap + c0 + e];
        i = i < 0 ? 0 : (i >= A.n ? A.n - 1 : i);
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
      const double q = (d0 * s00 + d1 * s10) * d0 + (d0 * s01 + d1 * s11) * d1;
      const double raw = al * exp(-0.5 * fmax(q, 0.0));
      const double a = fmin(A.c.alpha_max, raw);
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
        Tr *= na;
        if (Tr < A.c.t_stop) live = false;
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

unsigned ev_blocks(int64_t threads) { return (unsigned)((threads + kRdT - 1) / kRdT); }

bool ev_finite(double x) { return fabs(x) <= 1e300; }

// the part of the camera view's configuration the evidence reads, checked as gc_render_depth_tiles checks it
int ev_cfg(gc_ctx* ctx, const gc_camview_cfg* h, EvCfg* c) {
  GC_CHECK_ARG(ctx, cfg_all<13>(h, ev_finite), "the configuration must be finite");
  GC_CHECK_ARG(ctx, h->near > 0.0 && h->far > h->near, "near must be > 0 and far > near");
  GC_CHECK_ARG(ctx, h->alpha_max > 0.0 && h->alpha_max <= 1.0, "alpha_max must be in (0, 1]");
  c->alpha_max = h->alpha_max; c->alpha_skip = h->alpha_skip; c->t_stop = h->t_stop; c->eps = h->eps;
  return GC_OK;
}

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
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "H and W must be in [1, 16384]");
  EvCfg c;
  if (int rc = ev_cfg(ctx, cfg, &c)) return rc;
  double hv[kRdMaxViews * kEvView];
  for (int v = 0; v < n_poses; ++v) {
    const double* T = h_T_cw + 16 * v;
    const double* K = h_intrinsics + 4 * v;
    for (int q = 0; q < 16; ++q) GC_CHECK_ARG(ctx, ev_finite(T[q]), "T_cw must be finite");
    for (int q = 0; q < 4; ++q) GC_CHECK_ARG(ctx, ev_finite(K[q]), "the intrinsics must be finite");
    for (int q = 0; q < 3; ++q) GC_CHECK_ARG(ctx, ev_finite(h_t_wb[3 * v + q]), "t_wb must be finite");
    GC_CHECK_ARG(ctx, K[0] > 0.0 && K[1] > 0.0, "fx and fy must be > 0");
    GC_CHECK_ARG(ctx, T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0, "the bottom row of T_cw must be (0, 0, 0, 1)");
    double* V = hv + kEvView * v;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) V[3 * r + k] = T[4 * r + k];
      V[9 + r] = T[4 * r + 3];
    }
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) {
        const double g = V[r] * V[k] + V[3 + r] * V[3 + k] + V[6 + r] * V[6 + k] - (r == k ? 1.0 : 0.0);  // R^T R - I
        GC_CHECK_ARG(ctx, fabs(g) <= 1e-9, "the 3 x 3 block of T_cw must be a rotation");
      }
    for (int q = 0; q < 4; ++q) V[12 + q] = K[q];
    for (int q = 0; q < 3; ++q) V[16 + q] = h_t_wb[3 * v + q];
    V[19] = 1.3 * fmax(K[2], (double)W - K[2]) / K[0];  // k_cam_prep's limx, limy
    V[20] = 1.3 * fmax(K[3], (double)H - K[3]) / K[1];
    V[21] = 0.0;
  }
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, batch->mu_world && batch->Sigma_world, "NULL batch field");
  GC_CHECK_ARG(ctx, splats->Sigmas_inv && splats->valid, "NULL splat field");
  GC_CHECK_ARG(ctx, d_dmeans_px && d_ddepths && d_dSigmas_inv, "NULL output buffer");
  hipStream_t st = ctx->stream;
  for (int v0 = 0; v0 < n_poses; v0 += kEvViewsPerLaunch) {
    const int nv = n_poses - v0 < kEvViewsPerLaunch ? n_poses - v0 : kEvViewsPerLaunch;
    EvViews views = {};
    for (int q = 0; q < nv * kEvView; ++q) views.v[q] = hv[v0 * kEvView + q];
    hipLaunchKernelGGL(k_ev_jvp, dim3(ev_blocks(n * nv)), dim3(kRdT), 0, st, n, v0, nv, *batch, views,
                       (const double*)splats->Sigmas_inv, (const uint8_t*)splats->valid, d_dmeans_px, d_ddepths,
                       d_dSigmas_inv);
    GC_LAUNCH_CHECK(ctx);
  }
  return GC_OK;
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
  GC_CHECK_ARG(ctx, n_poses >= 1 && n_poses <= kRdMaxViews, "n_poses must be in [1, 32]");
  GC_CHECK_ARG(ctx, tile_size >= 1 && tile_size <= kEvMaxTile, "tile_size must be in [1, 16]: a thread owns one pixel");
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "H and W must be in [1, 16384]");
  GC_CHECK_ARG(ctx, H % tile_size == 0 && W % tile_size == 0, "H and W must be multiples of tile_size");
  GC_CHECK_ARG(ctx, cap >= 1 && cap <= kRdMaxCap, "cap must be in [1, 256]");
  GC_CHECK_ARG(ctx, n >= 0, "n must be >= 0");
  GC_CHECK_ARG(ctx, cfg != nullptr, "NULL configuration");
  EvRasterArgs A;
  if (int rc = ev_cfg(ctx, cfg, &A.c)) return rc;
  GC_CHECK_ARG(ctx, depth_model == 0 || depth_model == 1, "depth_model must be 0 (linear) or 1 (quadratic)");
  GC_CHECK_ARG(ctx, ev_finite(sigma0) && ev_finite(slope) && ev_finite(min_depth) && ev_finite(max_depth) &&
                        ev_finite(eps_lift) && (!use_robust || ev_finite(robust_nu)),
               "the evidence parameters must be finite");
  GC_CHECK_ARG(ctx, sigma0 > 0.0 && slope >= 0.0, "depth_sigma0 must be > 0 and depth_sigma_slope >= 0");
  GC_CHECK_ARG(ctx, min_depth >= 0.0 && max_depth > min_depth, "the depth limits must satisfy 0 <= min < max");
  GC_CHECK_ARG(ctx, !use_robust || robust_nu > 0.0, "robust_nu must be > 0");
  GC_CHECK_ARG(ctx, eps_lift >= 0.0, "eps_lift must be >= 0");
  GC_CHECK_ARG(ctx, d_L_pose && d_h_pose && d_parts, "NULL output buffer");
  TileGrid G;
  G.tiles_x = W / tile_size;
  G.T = G.tiles_x * (H / tile_size);
  G.ts = tile_size;
  G.oy0 = G.ox0 = 0;
  const int64_t segs = (int64_t)n_poses * G.T;
  GC_CHECK_ARG(ctx, segs < ((int64_t)1 << 31) && (n == 0 || segs < ((int64_t)1 << 32) / n),
               "n_poses * tiles * n must be below 2^32");
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
