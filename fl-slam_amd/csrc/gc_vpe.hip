// gc_vpe.hip — VisualPoseEvidence on the device, batched over hypotheses (the current
// PrimitiveMap path: view -> OT association -> pose evidence).
//
//  visual_pose_evidence                backend/operators/visual_pose_evidence.py:261-436
//  _compute_translation_evidence_wls   :74-162
//  _compute_rotation_evidence_vmf      :165-253
//  measurement means / directions / κ  backend/structures/measurement_batch.py:389-411
//
// The reference runs the operator once per hypothesis with the same association; only the
// linearisation pose differs. Two passes:
//
//  k_vpe_collapse  once per call, pose-independent. A group of 8 lanes per measurement row gathers
//                  the row's K candidates from the view pool (all indexed loads of a row in flight
//                  together), collapses them to one 128-B record [Λ_i (9) | m_i (3) | s_i | c̄_i (3)]
//                  and accumulates the pose-independent sums (kQ values, below).
//  k_vpe_hyp       one workgroup per hypothesis adds the per-workgroup partials in a fixed order
//                  (sum_partials; k_vpe_totals does only that when H = 0) and streams the N
//                  records (shared by all H, L2-resident):
//                    h_trans    = A − Σ_i s_i Λ_i R m_i
//                    cost_trans = V + Σ_i s_i yᵀ Λ_i y,  y = c̄_i/s_i − R m_i − t
//                    cost_rot   = W − ⟨R, S⟩
//                  then one lane does svd3, the determinant fix and so3_log, and the workgroup writes
//                  the 22 x 22 embedding.
//
// Reproducibility: no floating-point atomics anywhere. Every sum is lane-local in index order, then
// the fixed-order sums of gc_blocksum.h (group_sum_xor, block_sum, sum_partials); the grid depends on N
// alone, so a result is bitwise the same from run to run and row h of a batch equals the single-pose call.
#include <hip/hip_runtime.h>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"

namespace gc {
namespace {

constexpr int kVpeMaxK = 16;
constexpr int kVpeT = 256;              // threads per workgroup, both passes
constexpr int kVpeGroup = 8;            // lanes per measurement row
constexpr int kVpeRows = kVpeT / kVpeGroup;  // rows per workgroup tile
constexpr int kVpeMaxGrid = 1024;       // collapse workgroups (each loops over row tiles)
constexpr int kRec = 16;                // doubles per row record (one 128-B line)
// pose-independent sums: L_trans (9, no lift) | S (9) | W | A (3) | V | Σ row_masses | n_valid_meas | n_valid_map
constexpr int kQ = 26;
constexpr int qL = 0, qS = 9, qW = 18, qA = 19, qV = 22, qM = 23, qNv = 24, qNm = 25;
// the second pass (sum_partials) gives each value one of 32 thread columns: eight chains of workgroups
constexpr int kVpeCols = 32;
static_assert(kQ <= kVpeCols, "one thread column per value");

__global__ void __launch_bounds__(kVpeT) k_vpe_collapse(
    int64_t N, int K, int L, const double* __restrict__ Lam, const double* __restrict__ tht,
    const double* __restrict__ eta, const uint8_t* __restrict__ valid, const double* __restrict__ resp,
    const int32_t* __restrict__ pool, const double* __restrict__ rowm, const double* __restrict__ vpos,
    const double* __restrict__ vdir, const double* __restrict__ vkap, const uint8_t* __restrict__ vvalid,
    int64_t V, double eps_lift, double eps_mass, double* __restrict__ rec, double* __restrict__ partial) {
  __shared__ double red[(kVpeT / 64) * kQ];
  double acc[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) acc[q] = 0.0;
  const int sub = threadIdx.x & (kVpeGroup - 1), grp = threadIdx.x / kVpeGroup;
  const int64_t tiles = (N + kVpeRows - 1) / kVpeRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kVpeRows + grp;
    const bool in = i < N;
    const bool vi = in && valid[i] != 0;
    // this lane's candidates k = sub, sub + 8: issue every indexed load before any use
    double pi[2] = {0.0, 0.0}, c[2][3] = {{0, 0, 0}, {0, 0, 0}}, d[2][3] = {{0, 0, 0}, {0, 0, 0}}, km[2] = {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = sub + u * kVpeGroup;
      if (vi && k < K) {
        int64_t j = pool[i * K + k];
        j = j < 0 ? 0 : (j > V - 1 ? V - 1 : j);  // the clamp of a JAX gather: never outside the view
        pi[u] = resp[i * K + k];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          c[u][q] = vpos[3 * j + q];
          d[u][q] = vdir[3 * j + q];
        }
        km[u] = vkap[j];
      }
    }
    double Lr[9], es[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 9; ++q) Lr[q] = 0.0;
    if (vi) {
      lifted3(Lam + 9 * i, eps_lift, Lr);
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int q = 0; q < 3; ++q) es[q] += eta[(i * L + l) * 3 + q];
    }
    const double kap = sqrt(es[0] * es[0] + es[1] * es[1] + es[2] * es[2]);
    const double mu[3] = {es[0] / (kap + eps_mass), es[1] / (kap + eps_mass), es[2] / (kap + eps_mass)};
    // s_i = Σ_k π, c̄_i = Σ_k π c over the row's lane group (every lane ends with the same values)
    double g[4] = {pi[0] + pi[1], pi[0] * c[0][0] + pi[1] * c[1][0], pi[0] * c[0][1] + pi[1] * c[1][1],
                   pi[0] * c[0][2] + pi[1] * c[1][2]};
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = group_sum_xor<kVpeGroup>(g[q]);
    const double s = g[0];
    if (vi) {
      const bool has = s != 0.0;
      const double cm[3] = {has ? g[1] / s : 0.0, has ? g[2] / s : 0.0, has ? g[3] / s : 0.0};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (sub + u * kVpeGroup < K) {
          const double w = pi[u] * sqrt(kap * km[u] + 1e-12);
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[qS + 3 * a + b] += w * d[u][a] * mu[b];
          acc[qW] += w;
          if (has) {
            const double dl[3] = {c[u][0] - cm[0], c[u][1] - cm[1], c[u][2] - cm[2]};
            double Ld[3];
            mat3_vec(Lr, dl, Ld);
            acc[qV] += pi[u] * dot3(dl, Ld);
          }
        }
      }
    }
    if (sub == 0 && in) {
      double m[3] = {0.0, 0.0, 0.0};
      if (vi) {
        solve3(Lr, tht + 3 * i, m);
        const double cb[3] = {g[1], g[2], g[3]};
        double Lc[3];
        mat3_vec(Lr, cb, Lc);
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[qL + q] += s * Lr[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[qA + q] += Lc[q];
        acc[qM] += rowm[i];
        acc[qNv] += 1.0;
      }
      double* r = rec + kRec * i;  // an invalid row's record is all zero: it adds nothing in pass 2
#pragma unroll
      for (int q = 0; q < 9; ++q) r[q] = Lr[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        r[9 + q] = m[q];
        r[13 + q] = vi ? g[1 + q] : 0.0;
      }
      r[12] = vi ? s : 0.0;
    }
  }
  // valid view entries (integers held in f64: exact)
  for (int64_t v = (int64_t)blockIdx.x * kVpeT + threadIdx.x; v < V; v += (int64_t)gridDim.x * kVpeT)
    acc[qNm] += vvalid[v] != 0 ? 1.0 : 0.0;
  block_sum_stage<kQ>(acc, red);
  if ((int)threadIdx.x < kQ)
    partial[(int64_t)blockIdx.x * kQ + threadIdx.x] = block_sum_total<kQ, kVpeT / 64>(red, threadIdx.x);
}

// H = 0: the totals alone (the certificate vector). sum_partials' order depends on G alone, so this
// kernel and k_vpe_hyp get the same bits.
__global__ void __launch_bounds__(kVpeT) k_vpe_totals(int G, const double* __restrict__ partial, double* __restrict__ tot_out) {
  __shared__ double stage[kVpeT];
  __shared__ double tot[kQ];
  sum_partials<kVpeCols, kVpeT>(G, partial, kQ, stage, tot);
  if ((int)threadIdx.x < kQ) tot_out[threadIdx.x] = tot[threadIdx.x];
}

__global__ void __launch_bounds__(kVpeT) k_vpe_hyp(int64_t N, const double* __restrict__ rec, int G,
                                                   const double* __restrict__ partial, double* __restrict__ tot_out,
                                                   const double* __restrict__ pose6, double eps_lift,
                                                   double* __restrict__ L_pose, double* __restrict__ h_pose,
                                                   double* __restrict__ parts) {
  __shared__ double stage[kVpeT];
  __shared__ double tot[kQ];
  __shared__ double red[(kVpeT / 64) * 4];
  __shared__ double out[GC_VPE_PARTS];
  const int h = blockIdx.x;
  sum_partials<kVpeCols, kVpeT>(G, partial, kQ, stage, tot);  // every hypothesis sums the partials itself: no launch between
  if (h == 0 && (int)threadIdx.x < kQ) tot_out[threadIdx.x] = tot[threadIdx.x];  // for the host's certificate
  const bool empty = tot[qNv] == 0.0 || tot[qNm] == 0.0;  // visual_pose_evidence.py:297-318
  double R[9];
  so3_exp(pose6 + 6 * h + 3, R);
  const double t[3] = {pose6[6 * h], pose6[6 * h + 1], pose6[6 * h + 2]};
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // Σ s Λ R m (3) | Σ s yᵀ Λ y
  if (!empty) {
    for (int64_t i = threadIdx.x; i < N; i += kVpeT) {
      const double* r = rec + kRec * i;
      double v[kRec];
#pragma unroll
      for (int q = 0; q < kRec; ++q) v[q] = r[q];
      const double s = v[12];
      if (s != 0.0) {
        double Rm[3], LRm[3], Ly[3];
        mat3_vec(R, v + 9, Rm);
        mat3_vec(v, Rm, LRm);
        const double y[3] = {v[13] / s - Rm[0] - t[0], v[14] / s - Rm[1] - t[1], v[15] / s - Rm[2] - t[2]};
        mat3_vec(v, y, Ly);
        acc[0] += s * LRm[0];
        acc[1] += s * LRm[1];
        acc[2] += s * LRm[2];
        acc[3] += s * dot3(y, Ly);
      }
    }
  }
  block_sum<4, kVpeT / 64>(acc, red);
  if (threadIdx.x == 0) {
    if (empty) {
      for (int q = 0; q < GC_VPE_PARTS; ++q) out[q] = 0.0;
    } else {
      double S[9], U[9], sv[3], Vm[9], Rsc[9], Rd[9], rv[3];
      double rs = 0.0;
      for (int q = 0; q < 9; ++q) {
        S[q] = tot[qS + q];
        rs += R[q] * S[q];
        out[q] = tot[qL + q] + ((q % 4 == 0) ? eps_lift : 0.0);
      }
      for (int q = 0; q < 3; ++q) out[9 + q] = tot[qA + q] - acc[q];
      svd3(S, U, sv, Vm);
      mat3_mul_nt(U, Vm, Rsc);
      if (det3(Rsc) < 0.0) {  // U diag(1, 1, -1) Vᵀ
        U[2] = -U[2]; U[5] = -U[5]; U[8] = -U[8];
        mat3_mul_nt(U, Vm, Rsc);
      }
      mat3_mul_nt(Rsc, R, Rd);
      so3_log(Rd, rv);
      for (int q = 0; q < 9; ++q) out[12 + q] = 0.0;
      for (int q = 0; q < 3; ++q) {
        out[12 + 4 * q] = sv[q] + eps_lift;
        out[21 + q] = (sv[q] + eps_lift) * rv[q];
      }
      out[24] = tot[qV] + acc[3];
      out[25] = tot[qW] - rs;
    }
  }
  __syncthreads();
  // the 22-D embedding: eps_lift I with L_trans at [0:3, 0:3] and L_rot at [3:6, 3:6]
  for (int e = threadIdx.x; e < 22 * 22; e += kVpeT) {
    const int r = e / 22, cc = e - 22 * r;
    double x = r == cc ? eps_lift : 0.0;
    if (!empty && r < 6 && cc < 6) {
      if (r < 3 && cc < 3) x = out[3 * r + cc];
      else if (r >= 3 && cc >= 3) x = out[12 + 3 * (r - 3) + (cc - 3)];
      else x = 0.0;
    }
    L_pose[(int64_t)h * 484 + e] = x;
  }
  if (threadIdx.x < 22) {
    const int q = threadIdx.x;
    h_pose[(int64_t)h * 22 + q] = (empty || q >= 6) ? 0.0 : (q < 3 ? out[9 + q] : out[21 + q - 3]);
  }
  if (threadIdx.x < GC_VPE_PARTS) parts[(int64_t)h * GC_VPE_PARTS + threadIdx.x] = out[threadIdx.x];
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_visual_pose_evidence(gc_ctx* ctx, int64_t N, int32_t K, int32_t n_lobes, const double* d_Lambdas,
                                const double* d_thetas, const double* d_etas, const uint8_t* d_valid,
                                const double* d_resp, const int32_t* d_pool_idx, const double* d_row_masses,
                                const gc_map_view* view, int32_t H, const double* d_pose6, double eps_lift,
                                double eps_mass, double* d_L_pose, double* d_h_pose, double* d_parts,
                                double* h_cert) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, N >= 0 && H >= 0, "N and H must be >= 0");
  GC_CHECK_ARG(ctx, K >= 1 && K <= kVpeMaxK, "K must be in [1, 16]");
  GC_CHECK_ARG(ctx, n_lobes >= 1 && n_lobes <= kMapMaxLobes, "n_lobes must be in [1, 8]");
  GC_CHECK_ARG(ctx, view && h_cert, "NULL argument");
  GC_CHECK_ARG(ctx, N == 0 || (d_Lambdas && d_thetas && d_etas && d_valid && d_resp && d_pool_idx && d_row_masses),
               "NULL measurement / association buffer");
  GC_CHECK_ARG(ctx, H == 0 || (d_pose6 && d_L_pose && d_h_pose && d_parts), "NULL pose / output buffer");
  const int64_t V = (int64_t)view->n_tiles * view->m_tile_view;
  GC_CHECK_ARG(ctx, view->n_tiles >= 1 && view->m_tile_view >= 1 && V < (int64_t)INT32_MAX, "bad view shape");
  GC_CHECK_ARG(ctx, view->positions && view->directions && view->kappas && view->valid_mask, "NULL view field");
  const int64_t tiles = (N + kVpeRows - 1) / kVpeRows;
  const int G = (int)(tiles < 1 ? 1 : (tiles > kVpeMaxGrid ? kVpeMaxGrid : tiles));
  double *rec, *partial, *tot;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        rec = c.take<double>(kRec * (size_t)(N > 0 ? N : 1));
        partial = c.take<double>((size_t)kQ * G);
        tot = c.take<double>(kQ);
      }))
    return rc;
  hipLaunchKernelGGL(k_vpe_collapse, dim3((unsigned)G), dim3(kVpeT), 0, ctx->stream, N, (int)K, (int)n_lobes,
                     d_Lambdas, d_thetas, d_etas, d_valid, d_resp, d_pool_idx, d_row_masses,
                     (const double*)view->positions, (const double*)view->directions, (const double*)view->kappas,
                     (const uint8_t*)view->valid_mask, V, eps_lift, eps_mass, rec, partial);
  GC_LAUNCH_CHECK(ctx);
  if (H > 0) {
    hipLaunchKernelGGL(k_vpe_hyp, dim3((unsigned)H), dim3(kVpeT), 0, ctx->stream, N, (const double*)rec, G,
                       (const double*)partial, tot, d_pose6, eps_lift, d_L_pose, d_h_pose, d_parts);
  } else {
    hipLaunchKernelGGL(k_vpe_totals, dim3(1), dim3(kVpeT), 0, ctx->stream, G, (const double*)partial, tot);
  }
  GC_LAUNCH_CHECK(ctx);
  double ht[4] = {0, 0, 0, 0};  // tot[qM .. qNm] are adjacent: Σ row_masses, n_valid_meas, n_valid_map
  GC_HIP(ctx, hipMemcpyAsync(ht, tot + qM, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (int rc_w = gc::wait_stream(ctx, ctx->stream, "a result download")) return rc_w;
  h_cert[0] = ht[1];
  h_cert[1] = ht[2];
  h_cert[2] = ht[0];
  h_cert[3] = ht[1] > 0.0 ? ht[0] / ht[1] : 0.0;
  return GC_OK;
}

}  // extern "C"
