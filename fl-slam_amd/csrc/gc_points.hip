// gc_points.hip — per-point kernels of the GC-SLAM v2 hot path (gfx950).
//
//  a1 PointBudgetResample   backend/operators/point_budget.py:50-221
//  a4 DeskewConstantTwist   backend/operators/deskew_constant_twist.py:31-117 (+ pipeline.py:589-593)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "gc_internal.h"
#include "gc_wgla.h"
#include "gc_budget.h"

namespace gc {

// =============================================================================== a1 budget
// Two-level deterministic reduction: 64 workgroups write [Σw_in, Σw_sel, Σw_sel²] partials, one
// thread finishes (gc_budget.h).
__global__ void __launch_bounds__(256) k_budget_partials(const double* __restrict__ w, int64_t n_in,
                                                         int64_t stride, double* part) {
  __shared__ double red[4];
  budget_partial_block(w, n_in, stride, blockIdx.x, part, red);
}

__global__ void k_budget_final(const double* __restrict__ part, int64_t n_in, int64_t n_cap, int64_t stride,
                               double* out) {
  if (threadIdx.x != 0) return;
  budget_final_values(part, n_in, n_cap, stride, out);
}

__global__ void k_budget_gather(const double* __restrict__ pts, const double* __restrict__ t,
                                const double* __restrict__ w, const uint8_t* __restrict__ ring,
                                const uint8_t* __restrict__ tag, int64_t n_in, int64_t n_cap,
                                int64_t stride, const double* __restrict__ scal, double* pts_o,
                                double* t_o, double* w_o, uint8_t* ring_o, uint8_t* tag_o,
                                int64_t* idx_o) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cap) return;
  const int64_t n_sel = (n_in + stride - 1) / stride;
  const bool sel = j < n_sel;
  const int64_t i = j * stride;
  pts_o[3 * j + 0] = sel ? pts[3 * i + 0] : 0.0;
  pts_o[3 * j + 1] = sel ? pts[3 * i + 1] : 0.0;
  pts_o[3 * j + 2] = sel ? pts[3 * i + 2] : 0.0;
  t_o[j] = sel ? t[i] : 0.0;
  w_o[j] = sel ? w[i] * scal[2] : 0.0;
  if (ring_o) ring_o[j] = (sel && ring) ? ring[i] : 0;
  if (tag_o) tag_o[j] = (sel && tag) ? tag[i] : 0;
  if (idx_o) idx_o[j] = sel ? i : -1;
}

// ============================================================================== a4 deskew
__global__ void __launch_bounds__(256) k_deskew(int64_t n, const double* __restrict__ pts,
                                                const double* __restrict__ t,
                                                const double* __restrict__ w, double t0, double t1,
                                                const double* __restrict__ xi, double* pts_o,
                                                double* w_o, double* partial) {
  __shared__ double red[4];
  const int h = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * kWG + threadIdx.x;
  double xr[6];
  for (int k = 0; k < 6; ++k) xr[k] = xi[6 * h + k];
  const double denom = fmax(t1 - t0, 1e-12);
  double wo = 0.0;
  if (j < n) {
    const double p[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
    const double alpha = (t[j] - t0) / denom;
    double q[3];
    deskew_point(p, alpha, xr, q);
    wo = w[j] * window_weight(t[j], t0, t1, 0.1 * denom);
    const int64_t o = (int64_t)h * n + j;
    pts_o[3 * o] = q[0]; pts_o[3 * o + 1] = q[1]; pts_o[3 * o + 2] = q[2];
    w_o[o] = wo;
  }
  const double s = wg_sum(wo, red);
  if (threadIdx.x == 0) partial[(int64_t)h * gridDim.x + blockIdx.x] = s;
}

// out[h] = Σ_c partial[h][c] (fixed order)
__global__ void k_sum_rows(const double* __restrict__ partial, int64_t cols, int rows, double* out) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= rows) return;
  double s = 0.0;
  for (int64_t c = 0; c < cols; ++c) s += partial[(int64_t)h * cols + c];
  out[h] = s;
}

__global__ void k_point_dirs(int64_t rows, const double* __restrict__ pts, double o0, double o1,
                             double o2, double eps, double* dirs) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  const double p[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
  const double o[3] = {o0, o1, o2};
  double d[3];
  direction(p, o, eps, d);
  dirs[3 * j] = d[0]; dirs[3 * j + 1] = d[1]; dirs[3 * j + 2] = d[2];
}

}  // namespace gc

using namespace gc;

namespace gc {
hipError_t launch_budget_stats(const double* d_w, int64_t n_in, int64_t n_cap, double* part, double* out,
                               hipStream_t st) {
  const int64_t stride = budget_stride(n_in, n_cap);
  hipLaunchKernelGGL(k_budget_partials, dim3(kBudgetBlocks), dim3(256), 0, st, d_w, n_in, stride, part);
  hipLaunchKernelGGL(k_budget_final, dim3(1), dim3(64), 0, st, (const double*)part, n_in, n_cap, stride, out);
  return hipGetLastError();
}
}  // namespace gc

extern "C" {

int32_t gc_budget_stats(gc_ctx* ctx, const double* d_w, int64_t n_in, int64_t n_cap, double* d_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, n_in > 0 && n_cap > 0, "n_in and n_cap must be positive");
  GC_CHECK_ARG(ctx, d_w && d_out, "NULL buffer");
  void* scr;
  if (int rc = gc::scratch(ctx, sizeof(double) * 3 * kBudgetBlocks, &scr)) return rc;
  GC_HIP(ctx, gc::launch_budget_stats(d_w, n_in, n_cap, (double*)scr, d_out, ctx->stream));
  return GC_OK;
}

int32_t gc_point_budget_resample(gc_ctx* ctx, const double* d_points, const double* d_t, const double* d_w,
                                 const uint8_t* d_ring, const uint8_t* d_tag, int64_t n_in, int64_t n_cap,
                                 double* d_points_out, double* d_t_out, double* d_w_out, uint8_t* d_ring_out,
                                 uint8_t* d_tag_out, int64_t* d_idx_out, double* d_scalars_out) {
  int32_t rc = gc_budget_stats(ctx, d_w, n_in, n_cap, d_scalars_out);
  if (rc) return rc;
  GC_CHECK_ARG(ctx, d_points && d_t && d_points_out && d_t_out && d_w_out, "NULL buffer");
  const int64_t stride = std::max<int64_t>(1, (n_in + n_cap - 1) / n_cap);
  hipLaunchKernelGGL(k_budget_gather, dim3((unsigned)((n_cap + 255) / 256)), dim3(256), 0, ctx->stream,
                     d_points, d_t, d_w, d_ring, d_tag, n_in, n_cap, stride, d_scalars_out, d_points_out,
                     d_t_out, d_w_out, d_ring_out, d_tag_out, d_idx_out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_deskew_constant_twist(gc_ctx* ctx, int32_t H, int64_t n, const double* d_points, const double* d_t,
                                 const double* d_w, double t0, double t1, const double* d_xi,
                                 double* d_points_out, double* d_w_out, double* d_sum_w_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, H > 0 && n > 0, "H and n must be positive");
  GC_CHECK_ARG(ctx, d_points && d_t && d_w && d_xi && d_points_out && d_w_out && d_sum_w_out, "NULL buffer");
  const int64_t blocks = (n + 255) / 256;
  void* scr;
  if (int rc = gc::scratch(ctx, sizeof(double) * blocks * H, &scr)) return rc;
  hipLaunchKernelGGL(k_deskew, dim3((unsigned)blocks, H), dim3(256), 0, ctx->stream, n, d_points, d_t, d_w, t0,
                     t1, d_xi, d_points_out, d_w_out, (double*)scr);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_sum_rows, dim3((H + 63) / 64), dim3(64), 0, ctx->stream, (const double*)scr, blocks, H,
                     d_sum_w_out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_point_directions(gc_ctx* ctx, int64_t rows, const double* d_points, const double* h_origin3,
                            double eps_mass, double* d_dirs_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  GC_CHECK_ARG(ctx, rows > 0 && d_points && h_origin3 && d_dirs_out, "bad arguments");
  hipLaunchKernelGGL(k_point_dirs, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, rows,
                     d_points, h_origin3[0], h_origin3[1], h_origin3[2], eps_mass, d_dirs_out);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
