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
// and the photometric pose evidence ("Photometric pose evidence"): the same raster carrying one
// luminance channel y = w . colour (with the vMF shading) in the place of the depth, alone or beside it.
//
//   gc_image_luminance      per pixel: an rgb8 image as the float32 luminance the evidence observes.
//   gc_camera_shade_jvp     per (pose, primitive): the luminance of gc_camera_splat_prep's colour row and
//                           its six tangents, the tangents of rd_vmf_shading towards the camera centre.
//   gc_photo_pose_evidence  k_ev_raster carrying (T, Y, dT[6], dY[6]).
//   gc_rgbd_pose_evidence   k_ev_raster carrying (T, D, Y, dT[6], dD[6], dY[6]): one pass over the lists for
//                           both evidences, two partial rows per (pose, tile).
//
// The tangent convention is visual_pose_evidence.py's (r = map - (R m + t), d/dt = -I, :89-99;
// R_delta = R_scatter R_pred^T, :234-238): t_wb' = t_wb + dt, R_wb' = Exp(dtheta) R_wb. No floating-point
// atomics: the outputs are bitwise reproducible from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_mapslot.h"
#include "gc_renderdev.h"

namespace gc {
namespace {

constexpr int kEvMaxTile = 16;  // a thread owns one pixel
constexpr int kEvRec = 44;      // a record: mean 2, Sigma^-1 4, alpha, depth, dmean 12, ddepth 6, dSigma^-1 18
constexpr int kEvRecBoth = 52;  // ... and behind it the luminance's six tangents, the luminance and one pad (16-B pairs)
constexpr int kEvChunk = 64;    // records staged per barrier pair: 22 KB of LDS (26 KB with both channels)
constexpr int kEvNV = GC_DEPTHEV_PARTIAL;
constexpr int kEvParts = GC_DEPTHEV_PARTS;
static_assert(kEvNV == 21 + 6 + 4 && kEvParts == 36 + 6 + 4, "gcslam.h");
static_assert(kEvMaxTile * kEvMaxTile == kRdT, "one thread per pixel of the largest tile");
static_assert(kRdT % 4 == 0 && kEvRec % 4 == 0 && kEvRecBoth % 4 == 0 && kEvChunk * 4 == kRdT,
              "four threads stage one record");

// the channels k_ev_raster carries: the depth, the luminance (in the depth's place of the record) or both
enum { kEvDepth = 1, kEvLum = 2, kEvBoth = 3 };

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

// The luminance y = (w0 r + w1 g) + w2 b of k_cam_prep's colour row (the forward's bits) and its six tangents
// (w . color) ds_k, laid out like k_ev_jvp. ds is the tangent of rd_vmf_shading at vd = c - mu with c the
// camera centre: dc = e_k for dt_k and e_k x (c - t_wb) for dtheta_k; n = |vd|, nv = n + 1e-12, v = vd / nv,
// dv = dc / nv - vd (vd . dc) / (n nv^2); ds = (1 / (1 + mean kappa)) (1 / L) sum_l exp(kappa_l (m_l . v - 1))
// kappa_l (m_l . dv) with m_l = eta_l / (kappa_l + 1e-12): the sum over the lobes is taken once, as the
// vector g = sum_l exp(.) kappa_l m_l, and ds_k = scale (g . dv_k).
__global__ __launch_bounds__(kRdT) void k_ev_shade_jvp(int64_t n, int v0, int n_views, gc_render_batch b, CamViews views,
                                                       int shade, double w0, double w1, double w2, const double* colors,
                                                       const uint8_t* valid, double* lum, double* dlum) {
  const int64_t gl = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (gl >= n * n_views) return;
  const int vl = (int)(gl / n);
  const int64_t i = gl - (int64_t)vl * n;
  const int64_t g = (int64_t)(v0 + vl) * n + i;
  double* od = dlum + 6 * g;
#pragma unroll
  for (int q = 0; q < 6; ++q) od[q] = 0.0;
  if (!valid[g]) {
    lum[g] = 0.0;
    return;
  }
  lum[g] = (w0 * colors[3 * g] + w1 * colors[3 * g + 1]) + w2 * colors[3 * g + 2];
  if (!shade) return;
  const double* V = views.v + kCamView * vl;
  double vd[3], rel[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    vd[q] = V[kCvCentre + q] - b.mu_world[3 * i + q];
    rel[q] = V[kCvCentre + q] - V[kCvTwb + q];
  }
  const double nn = sqrt(vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2]), nv = nn + 1e-12;
  const double u0 = vd[0] / nv, u1 = vd[1] / nv, u2 = vd[2] / nv;
  const int L = b.n_lobes;
  double gv[3] = {0.0, 0.0, 0.0}, kappa_sum = 0.0;
  for (int l = 0; l < L; ++l) {
    const double e0 = b.eta[(i * L + l) * 3], e1 = b.eta[(i * L + l) * 3 + 1], e2 = b.eta[(i * L + l) * 3 + 2];
    const double kap = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    const double nm = kap + 1e-12;
    const double m0 = e0 / nm, m1 = e1 / nm, m2 = e2 / nm;
    const double ek = exp(kap * (m0 * u0 + m1 * u1 + m2 * u2 - 1.0)) * kap;
    gv[0] += ek * m0;
    gv[1] += ek * m1;
    gv[2] += ek * m2;
    kappa_sum += kap;
  }
  const double scale = (1.0 / (1.0 + kappa_sum / (double)L)) * (1.0 / (double)L);
  const double wc = (w0 * b.color[3 * i] + w1 * b.color[3 * i + 1]) + w2 * b.color[3 * i + 2];
  const double inv = 1.0 / nv, back = 1.0 / (nn * nv * nv);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double dc[3];
    if (k < 3) {
      dc[0] = dc[1] = dc[2] = 0.0;
      dc[k] = 1.0;
    } else {
      const int a = k - 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
      // e_a x rel: component a1 is -rel[a2], component a2 is rel[a1]
      dc[a] = 0.0;
      dc[a1] = -rel[a2];
      dc[a2] = rel[a1];
    }
    const double along = (vd[0] * dc[0] + vd[1] * dc[1] + vd[2] * dc[2]) * back;
    const double dv0 = dc[0] * inv - vd[0] * along, dv1 = dc[1] * inv - vd[1] * along, dv2 = dc[2] * inv - vd[2] * along;
    od[k] = wc * (scale * (gv[0] * dv0 + gv[1] * dv1 + gv[2] * dv2));
  }
}

// an (H, W, 3) rgb8 image as the float32 luminance ((w0 R + w1 G) + w2 B) / 255, the sum in f64
__global__ __launch_bounds__(kRdT) void k_ev_luminance(int64_t px, const uint8_t* rgb, double w0, double w1, double w2,
                                                       float* lum) {
  const int64_t i = (int64_t)blockIdx.x * kRdT + threadIdx.x;
  if (i >= px) return;
  const double r = (double)rgb[3 * i], g = (double)rgb[3 * i + 1], bl = (double)rgb[3 * i + 2];
  lum[i] = (float)(((w0 * r + w1 * g) + w2 * bl) / 255.0);
}

// ------------------------------------------------------------------------------------------------
// the evidence raster
// ------------------------------------------------------------------------------------------------

// the part of the camera view's configuration the evidence reads (from a checked CamCfg), then its own: the
// depth's, and the luminance's (sigma_y, nu_y, robust_y)
struct EvCfg {
  double alpha_max, alpha_skip, t_stop, eps;
  double sigma0, slope, dmin, dmax, nu;
  int quadratic, robust;
  double sigma_y, nu_y;
  int robust_y;
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
  double *partial, *residual, *weight;  // partial: a row per segment and channel, the depth's rows first
  // the luminance channel
  const double *lums, *dlums;
  const float* obs_y;
  double *render_y, *residual_y, *weight_y;
};

// a used pixel's 31 values: the upper triangle of w J J^T by rows, w J r, w r^2, 1, the coverage, w
GC_DEV void ev_pixel_values(const double (&J)[6], double r, double w, double cover, double (&val)[kEvNV]) {
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
}

// One workgroup per (pose, tile), thread p the pixel p of the row-major tile (p < ts^2 <= 256). The list is
// staged kEvChunk records at a time (four threads per record), a barrier on either side; every lane reads
// the same record per step. A wave whose pixels have all stopped skips the arithmetic but keeps the
// barriers; the workgroup leaves the list once every pixel has stopped.
//
// MODE names the channels carried beside T and dT: kEvDepth (D, dD: the record's value and tangents are the
// depth's), kEvLum (Y, dY: the same record with the luminance in the depth's place) or kEvBoth (both; the
// luminance and its tangents follow the depth record). q, the exponential, dq and da are computed once per
// (splat, tangent) whatever the channels; a channel's arithmetic is the same in every instantiation that
// carries it.
template <int MODE>
__global__ __launch_bounds__(kRdT) void k_ev_raster(EvRasterArgs A) {
  constexpr bool kD = (MODE & kEvDepth) != 0, kY = (MODE & kEvLum) != 0;
  constexpr int kRec = (kD && kY) ? kEvRecBoth : kEvRec;
  constexpr int kYAt = kD ? kEvRec + 6 : 7, kDYAt = kD ? kEvRec : 20;  // the luminance and its tangents in a record
  __shared__ double rec[kEvChunk * kRec];
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
  double Tr = 1.0, D = 0.0, Y = 0.0, dT[6], dD[6], dY[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) dT[k] = dD[k] = dY[k] = 0.0;
  bool live = own;
  for (int c0 = 0; c0 < m; c0 += kEvChunk) {
    const int mc = m - c0 < kEvChunk ? m - c0 : kEvChunk;
    if (c0 > 0 && !__syncthreads_or(live ? 1 : 0)) break;  // also the barrier before rec is overwritten
    {
      const int e = threadIdx.x >> 2, part = threadIdx.x & 3;
      if (e < mc) {
        const int64_t i = rd_list_index(A.indices[seg * A.cap + c0 + e], A.n);
        const int64_t r = v * A.n + i;
        double* o = rec + kRec * e;
        if (part == 0) {
          o[0] = A.means[2 * r];
          o[1] = A.means[2 * r + 1];
#pragma unroll
          for (int q = 0; q < 4; ++q) o[2 + q] = A.Sinv[4 * r + q];
          o[6] = A.alphas[i];
          if constexpr (kD) o[7] = A.depths[r];
          if constexpr (kY) {
            o[kYAt] = A.lums[r];
#pragma unroll
            for (int q = 0; q < 6; ++q) o[kDYAt + q] = A.dlums[6 * r + q];
            if constexpr (kD) o[kEvRecBoth - 1] = 0.0;
          }
        } else if (part == 1) {
#pragma unroll
          for (int q = 0; q < 12; ++q) o[8 + q] = A.dmeans[12 * r + q];
        } else if (part == 2) {
          if constexpr (kD) {
#pragma unroll
            for (int q = 0; q < 6; ++q) o[20 + q] = A.ddepths[6 * r + q];
          }
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
      const double* o = rec + kRec * j;
      // first is the record's own value: the depth, or the luminance where the depth is not carried
      const double mx = o[0], my = o[1], s00 = o[2], s01 = o[3], s10 = o[4], s11 = o[5], al = o[6], first = o[7];
      const double d0 = px - mx, d1 = py - my;
      const double q = rd_quad(d0, d1, s00, s01, s10, s11);
      double raw, a;
      cam_step_alpha(al, q, A.c.alpha_max, raw, a);
      if (live && a >= A.c.alpha_skip) {
        const bool flat = raw > A.c.alpha_max || q < 0.0;
        const double g0 = s00 * d0 + s01 * d1, g1 = s10 * d0 + s11 * d1;
        const double d00 = d0 * d0, d01 = 2.0 * d0 * d1, d11 = d1 * d1;
        const double Ta = Tr * a, na = 1.0 - a;
        const double dep = first, lum = kD ? o[kYAt] : first;  // each is read only where its channel is carried
        const double az = a * dep, Tz = Tr * dep, ay = a * lum, Ty = Tr * lum;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double dq = -2.0 * (g0 * o[8 + 2 * k] + g1 * o[9 + 2 * k]) +
                            (o[26 + 3 * k] * d00 + o[27 + 3 * k] * d01 + o[28 + 3 * k] * d11);
          const double da = flat ? 0.0 : -0.5 * a * dq;
          if constexpr (kD) dD[k] += dT[k] * az + Tz * da + Ta * o[20 + k];
          if constexpr (kY) dY[k] += dT[k] * ay + Ty * da + Ta * o[kDYAt + k];
          dT[k] = dT[k] * na - Tr * da;
        }
        if constexpr (kD) D += Ta * dep;
        if constexpr (kY) Y += Ta * lum;
        if (cam_step_through(Tr, a, A.c.t_stop)) live = false;
      }
    }
  }
  // the pixel's evidence, a channel at a time: 31 values and one fixed-order workgroup sum each
  const int64_t at = (v * A.H + row) * A.W + col;
  const double cover = own ? A.alpha_img[at] : 0.0;
  if constexpr (kD) {
    double val[kEvNV];
#pragma unroll
    for (int q = 0; q < kEvNV; ++q) val[q] = 0.0;
    double r_out = 0.0, w_out = 0.0;
    if (own) {
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
        ev_pixel_values(J, r, w, cover, val);
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
  if constexpr (kY) {
    double val[kEvNV];
#pragma unroll
    for (int q = 0; q < kEvNV; ++q) val[q] = 0.0;
    double r_out = 0.0, w_out = 0.0, y_out = 0.0;
    if (own) {
      const double obs = (double)A.obs_y[(int64_t)row * A.W + col];
      const bool covered = cover > A.c.eps;
      if (covered) y_out = Y / cover;
      if (fabs(obs) < HUGE_VAL && covered) {
        const double r = y_out - obs;
        const double sg = A.c.sigma_y;
        const double rs = r / sg;
        const double u = A.c.robust_y ? (A.c.nu_y + 1.0) / (A.c.nu_y + rs * rs) : 1.0;
        const double w = cover * u / (sg * sg);
        const double ia2 = 1.0 / (cover * cover);
        double J[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) J[k] = (dY[k] * cover + Y * dT[k]) * ia2;
        ev_pixel_values(J, r, w, cover, val);
        r_out = r;
        w_out = w;
      }
      if (A.render_y) A.render_y[at] = y_out;
      if (A.residual_y) A.residual_y[at] = r_out;
      if (A.weight_y) A.weight_y[at] = w_out;
    }
    __syncthreads();
    block_sum<kEvNV, kRdT / 64>(val, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < kEvNV; ++q) A.partial[((kD ? (int64_t)gridDim.x : 0) + seg) * kEvNV + q] = val[q];
    }
  }
}

// one workgroup per pose: the tiles in a fixed order, then L_pose, h_pose and the parts row (rows of
// parts_stride values: the joint evidence keeps two rows per pose)
__global__ __launch_bounds__(kRdT) void k_ev_final(int G, const double* partial, double eps_lift, int accumulate,
                                                   double* L_pose, double* h_pose, double* parts, int parts_stride) {
  __shared__ double stage[kRdT], tot[32];
  const int v = blockIdx.x;
  sum_partials<32, kRdT>(G, partial + (int64_t)v * G * kEvNV, kEvNV, stage, tot);
  double* L = L_pose + (int64_t)v * 484;
  double* h = h_pose + (int64_t)v * 22;
  double* P = parts + (int64_t)v * parts_stride;
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

// what an evidence entry takes for a channel: NULL where the entry does not carry it
struct EvDepthIn {
  const double *ddepths, *depth_img;
  const float* obs;
  int model;
  double sigma0, slope, dmin, dmax;
  int robust;
  double nu;
  double *residual, *weight;
};
struct EvLumIn {
  const double *lum, *dlum;
  const float* obs;
  double sigma;
  int robust;
  double nu;
  double *render, *residual, *weight;
};

// The three evidence entries: every check, then the raster of the channels given and one k_ev_final per
// channel, the depth's first. The second of two adds into what the first wrote, so the lift is added once.
int ev_evidence(gc_ctx* ctx, const EvDepthIn* dp, const EvLumIn* lp, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                const double* d_dmeans_px, const double* d_dSigmas_inv, int32_t H, int32_t W, int32_t tile_size, int32_t cap,
                const gc_camview_cfg* cfg, const int32_t* d_tile_counts, const int32_t* d_tile_indices, const double* d_alpha,
                double eps_lift, int32_t accumulate, double* d_L_pose, double* d_h_pose, double* d_parts) {
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
  EvRasterArgs A = {};
  A.c.alpha_max = vc.alpha_max; A.c.alpha_skip = vc.alpha_skip; A.c.t_stop = vc.t_stop; A.c.eps = vc.eps;
  if (dp) {
    GC_CHECK_ARG(ctx, dp->model == 0 || dp->model == 1, "depth_model must be 0 (linear) or 1 (quadratic)");
    GC_CHECK_ARG(ctx, rd_finite(dp->sigma0) && rd_finite(dp->slope) && rd_finite(dp->dmin) && rd_finite(dp->dmax) &&
                          rd_finite(eps_lift) && (!dp->robust || rd_finite(dp->nu)),
                 "the evidence parameters must be finite");
    GC_CHECK_ARG(ctx, dp->sigma0 > 0.0 && dp->slope >= 0.0, "depth_sigma0 must be > 0 and depth_sigma_slope >= 0");
    GC_CHECK_ARG(ctx, dp->dmin >= 0.0 && dp->dmax > dp->dmin, "the depth limits must satisfy 0 <= min < max");
    GC_CHECK_ARG(ctx, !dp->robust || dp->nu > 0.0, "robust_nu must be > 0");
  }
  if (lp) {
    GC_CHECK_ARG(ctx, rd_finite(lp->sigma) && rd_finite(eps_lift) && (!lp->robust || rd_finite(lp->nu)),
                 "the evidence parameters must be finite");
    GC_CHECK_ARG(ctx, lp->sigma > 0.0, "sigma must be > 0");
    GC_CHECK_ARG(ctx, !lp->robust || lp->nu > 0.0, "robust_nu must be > 0");
  }
  GC_CHECK_ARG(ctx, eps_lift >= 0.0, "eps_lift must be >= 0");
  GC_CHECK_ARG(ctx, d_L_pose && d_h_pose && d_parts, "NULL output buffer");
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)n_poses * H * W;
  const int stride = (dp && lp) ? 2 * kEvParts : kEvParts;
  double* const parts_y = d_parts + (dp ? kEvParts : 0);
  // one k_ev_final per channel given, over the T tiles' rows of its partial sums
  auto finals = [&](int T, const double* partial_d, const double* partial_y) -> int {
    if (dp) {
      hipLaunchKernelGGL(k_ev_final, dim3((unsigned)n_poses), dim3(kRdT), 0, st, T, partial_d, eps_lift,
                         (int)(accumulate != 0), d_L_pose, d_h_pose, d_parts, stride);
      GC_LAUNCH_CHECK(ctx);
    }
    if (lp) {
      hipLaunchKernelGGL(k_ev_final, dim3((unsigned)n_poses), dim3(kRdT), 0, st, T, partial_y, eps_lift,
                         (int)(dp || accumulate != 0), d_L_pose, d_h_pose, parts_y, stride);
      GC_LAUNCH_CHECK(ctx);
    }
    return GC_OK;
  };
  if (n == 0) {  // no raster over an empty range: the sums over no tile
    double* const images[5] = {dp ? dp->residual : nullptr, dp ? dp->weight : nullptr, lp ? lp->render : nullptr,
                               lp ? lp->residual : nullptr, lp ? lp->weight : nullptr};
    for (double* im : images)
      if (im) GC_HIP(ctx, hipMemsetAsync(im, 0, sizeof(double) * px, st));
    return finals(0, nullptr, nullptr);
  }
  GC_CHECK_ARG(ctx, splats && splats->means_px && splats->Sigmas_inv && splats->alphas && (!dp || splats->depths),
               "NULL splat field");
  GC_CHECK_ARG(ctx, d_dmeans_px && d_dSigmas_inv && (!dp || dp->ddepths) && (!lp || (lp->lum && lp->dlum)),
               "NULL tangent array");
  GC_CHECK_ARG(ctx, d_tile_counts && d_tile_indices && d_alpha && (!dp || (dp->depth_img && dp->obs)) && (!lp || lp->obs),
               "NULL input buffer");
  double* partial;  // a row per segment and channel, the depth's rows first
  if (int rc = carve_scratch(ctx, [&](Carver& cv) { partial = cv.take<double>((size_t)segs * kEvNV * (dp && lp ? 2 : 1)); }))
    return rc;
  const double* partial_y = partial + (dp ? (size_t)segs * kEvNV : 0);
  A.n = n; A.G = G; A.H = H; A.W = W; A.cap = cap;
  A.means = splats->means_px; A.Sinv = splats->Sigmas_inv; A.alphas = splats->alphas;
  A.dmeans = d_dmeans_px; A.dSinv = d_dSigmas_inv;
  A.indices = d_tile_indices; A.counts = d_tile_counts;
  A.alpha_img = d_alpha; A.partial = partial;
  if (dp) {
    A.c.sigma0 = dp->sigma0; A.c.slope = dp->slope; A.c.dmin = dp->dmin; A.c.dmax = dp->dmax;
    A.c.nu = dp->robust ? dp->nu : 0.0;
    A.c.quadratic = dp->model; A.c.robust = dp->robust != 0;
    A.depths = splats->depths; A.ddepths = dp->ddepths; A.depth_img = dp->depth_img; A.obs = dp->obs;
    A.residual = dp->residual; A.weight = dp->weight;
  }
  if (lp) {
    A.c.sigma_y = lp->sigma; A.c.nu_y = lp->robust ? lp->nu : 0.0; A.c.robust_y = lp->robust != 0;
    A.lums = lp->lum; A.dlums = lp->dlum; A.obs_y = lp->obs;
    A.render_y = lp->render; A.residual_y = lp->residual; A.weight_y = lp->weight;
  }
  if (dp && lp) hipLaunchKernelGGL(k_ev_raster<kEvBoth>, dim3((unsigned)segs), dim3(kRdT), 0, st, A);
  else if (dp) hipLaunchKernelGGL(k_ev_raster<kEvDepth>, dim3((unsigned)segs), dim3(kRdT), 0, st, A);
  else hipLaunchKernelGGL(k_ev_raster<kEvLum>, dim3((unsigned)segs), dim3(kRdT), 0, st, A);
  GC_LAUNCH_CHECK(ctx);
  return finals((int)G.T, partial, partial_y);
}

// the checks gc_camera_splat_jvp and gc_camera_shade_jvp share, and the packed views
int ev_jvp_views(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_poses, const double* h_T_cw,
                 const double* h_t_wb, const double* h_intrinsics, int32_t H, int32_t W, const gc_camview_cfg* cfg,
                 const gc_cam_splats* splats, CamCfg* c, double* hv) {
  GC_CHECK_ARG(ctx, batch && h_T_cw && h_t_wb && h_intrinsics && cfg && splats, "NULL argument");
  GC_CHECK_ARG(ctx, n >= 0 && n <= ((int64_t)1 << 24), "n must be in [0, 2^24]");
  GC_CHECK_ARG(ctx, n_poses >= 1 && n_poses <= kRdMaxViews, "n_poses must be in [1, 32]");
  if (int rc = cam_cfg(ctx, cfg, c)) return rc;
  return cam_pack_views(ctx, n_poses, h_T_cw, h_intrinsics, h_t_wb, H, W, hv);
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
  CamCfg c;
  double hv[kRdMaxViews * kCamView];
  if (int rc = ev_jvp_views(ctx, batch, n, n_poses, h_T_cw, h_t_wb, h_intrinsics, H, W, cfg, splats, &c, hv)) return rc;
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

int32_t gc_camera_shade_jvp(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_poses, const double* h_T_cw,
                            const double* h_t_wb, const double* h_intrinsics, int32_t H, int32_t W,
                            const gc_camview_cfg* cfg, const gc_cam_splats* splats, const double* h_weights, double* d_lum,
                            double* d_dlum) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  CamCfg c;
  double hv[kRdMaxViews * kCamView];
  if (int rc = ev_jvp_views(ctx, batch, n, n_poses, h_T_cw, h_t_wb, h_intrinsics, H, W, cfg, splats, &c, hv)) return rc;
  GC_CHECK_ARG(ctx, h_weights != nullptr, "NULL argument");
  GC_CHECK_ARG(ctx, rd_finite(h_weights[0]) && rd_finite(h_weights[1]) && rd_finite(h_weights[2]),
               "the luminance weights must be finite");
  GC_CHECK_ARG(ctx, batch->n_lobes >= 1 && batch->n_lobes <= kMapMaxLobes, "n_lobes must be in [1, 8]");
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(ctx, batch->mu_world && batch->eta && batch->color, "NULL batch field");
  GC_CHECK_ARG(ctx, splats->colors && splats->valid, "NULL splat field");
  GC_CHECK_ARG(ctx, d_lum && d_dlum, "NULL output buffer");
  hipStream_t st = ctx->stream;
  const double w0 = h_weights[0], w1 = h_weights[1], w2 = h_weights[2];
  return cam_each_launch(ctx, n_poses, hv, [&](int v0, int nv, const CamViews& views) {
    hipLaunchKernelGGL(k_ev_shade_jvp, dim3(rd_blocks(n * nv)), dim3(kRdT), 0, st, n, v0, nv, *batch, views, (int)c.shade,
                       w0, w1, w2, (const double*)splats->colors, (const uint8_t*)splats->valid, d_lum, d_dlum);
  });
}

int32_t gc_image_luminance(gc_ctx* ctx, const uint8_t* d_rgb8, int32_t H, int32_t W, const double* h_weights,
                           float* d_lum) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, d_rgb8 && h_weights && d_lum, "NULL argument");
  GC_CHECK_ARG(ctx, H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "H and W must be in [1, 16384]");
  GC_CHECK_ARG(ctx, rd_finite(h_weights[0]) && rd_finite(h_weights[1]) && rd_finite(h_weights[2]),
               "the luminance weights must be finite");
  const int64_t px = (int64_t)H * W;
  hipLaunchKernelGGL(k_ev_luminance, dim3(rd_blocks(px)), dim3(kRdT), 0, ctx->stream, px, d_rgb8, h_weights[0], h_weights[1],
                     h_weights[2], d_lum);
  GC_LAUNCH_CHECK(ctx);
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
  const EvDepthIn dp = {d_ddepths, d_depth,   d_depth_obs, depth_model, sigma0,     slope,
                        min_depth, max_depth, use_robust,  robust_nu,   d_residual, d_weight};
  return ev_evidence(ctx, &dp, nullptr, n_poses, n, splats, d_dmeans_px, d_dSigmas_inv, H, W, tile_size, cap, cfg,
                     d_tile_counts, d_tile_indices, d_alpha, eps_lift, accumulate, d_L_pose, d_h_pose, d_parts);
}

int32_t gc_photo_pose_evidence(gc_ctx* ctx, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                               const double* d_dmeans_px, const double* d_dSigmas_inv, const double* d_lum,
                               const double* d_dlum, int32_t H, int32_t W, int32_t tile_size, int32_t cap,
                               const gc_camview_cfg* cfg, const int32_t* d_tile_counts, const int32_t* d_tile_indices,
                               const double* d_alpha, const float* d_lum_obs, double sigma, int32_t use_robust,
                               double robust_nu, double eps_lift, int32_t accumulate, double* d_L_pose, double* d_h_pose,
                               double* d_parts, double* d_lum_render, double* d_residual, double* d_weight) {
  const EvLumIn lp = {d_lum, d_dlum, d_lum_obs, sigma, use_robust, robust_nu, d_lum_render, d_residual, d_weight};
  return ev_evidence(ctx, nullptr, &lp, n_poses, n, splats, d_dmeans_px, d_dSigmas_inv, H, W, tile_size, cap, cfg,
                     d_tile_counts, d_tile_indices, d_alpha, eps_lift, accumulate, d_L_pose, d_h_pose, d_parts);
}

int32_t gc_rgbd_pose_evidence(gc_ctx* ctx, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                              const double* d_dmeans_px, const double* d_ddepths, const double* d_dSigmas_inv,
                              const double* d_lum, const double* d_dlum, int32_t H, int32_t W, int32_t tile_size,
                              int32_t cap, const gc_camview_cfg* cfg, const int32_t* d_tile_counts,
                              const int32_t* d_tile_indices, const double* d_alpha, const double* d_depth,
                              const float* d_depth_obs, int32_t depth_model, double sigma0, double slope, double min_depth,
                              double max_depth, int32_t depth_use_robust, double depth_robust_nu, const float* d_lum_obs,
                              double lum_sigma, int32_t lum_use_robust, double lum_robust_nu, double eps_lift,
                              int32_t accumulate, double* d_L_pose, double* d_h_pose, double* d_parts, double* d_residual,
                              double* d_weight, double* d_lum_render, double* d_lum_residual, double* d_lum_weight) {
  const EvDepthIn dp = {d_ddepths, d_depth,   d_depth_obs,      depth_model,     sigma0,     slope,
                        min_depth, max_depth, depth_use_robust, depth_robust_nu, d_residual, d_weight};
  const EvLumIn lp = {d_lum,           d_dlum,       d_lum_obs,      lum_sigma,   lum_use_robust,
                      lum_robust_nu,   d_lum_render, d_lum_residual, d_lum_weight};
  return ev_evidence(ctx, &dp, &lp, n_poses, n, splats, d_dmeans_px, d_dSigmas_inv, H, W, tile_size, cap, cfg,
                     d_tile_counts, d_tile_indices, d_alpha, eps_lift, accumulate, d_L_pose, d_h_pose, d_parts);
}

}  // extern "C"
