// gc_assoc.hip — map view extraction and OT association on the device.
//
//  extract_atlas_map_view      backend/structures/primitive_map.py:356-451 (+ :304-322, :475-498)
//  associate_primitives_ot     backend/operators/primitive_association.py:239-553
//                              (+ _compute_sparse_cost_matrix_jax :152-197, _A_vmf_vec_jax :141-149,
//                               _sinkhorn_unbalanced_fixed_k_jax :105-138, tiling.py:148-186)
//
// View: one segmented stable radix sort ranks each view tile's slots by weight (invalid last,
// ties by slot), then one thread per view entry gathers it and evaluates the info-form means /
// covariances and the vMF resultant. Association: one wave per measurement row evaluates the
// cost of its whole stencil pool (n_stencil x m_tile_view candidates, 64 lanes strided), keeps a
// lane-local sorted top-K by (cost, pool position) — exactly the order of the reference's stable
// sort on cost — and merges the 64 lists with K wave-argmin rounds. The fixed-iteration unbalanced
// Sinkhorn couples all rows through the column sums, so it runs in one 1024-thread workgroup with
// fixed-order block reductions (deterministic), the N x K kernel matrix streamed from L2.
#include <hip/hip_runtime.h>
#include "gc_blocksum.h"
#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"
#include "gc_sort.h"

namespace gc {
namespace {

constexpr int kMaxK = 16;          // k_assoc supported
constexpr int kMaxStencil = 128;   // n_z * n_xy stencil tiles per row
constexpr int kSinkT = 1024;       // Sinkhorn workgroup

struct OTCfg {
  int K, iters, row_min, wprop, r_xy, r_z;
  double beta, eps, tau_a, tau_b, eps_mass, h_tile, lam, eps_lift;
  int64_t seq;
};

// ---- view
__global__ void k_view_keys(gc_primitive_map map, int64_t m_tile, const int64_t* __restrict__ dense, int T,
                            double* keys, int32_t* vals, int* offsets) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= T) offsets[i] = (int)(i * m_tile);  // segment t = [t m_tile, (t+1) m_tile)
  if (i >= (int64_t)T * m_tile) return;
  const int t = (int)(i / m_tile);
  const int64_t s = i - (int64_t)t * m_tile;
  const int64_t d = dense[t];
  double key = 1e30;  // -score of an invalid slot (score -1e30)
  if (d >= 0) {
    const int64_t g = d * m_tile + s;
    if (mValid(map, g)) key = -mW(map, g);
  }
  keys[i] = key;
  vals[i] = (int32_t)s;
}

__global__ void k_view_gather(gc_primitive_map map, int64_t m_tile, const int64_t* __restrict__ dense,
                              const int32_t* __restrict__ order, gc_map_view V, double eps_lift, double eps_mass) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = V.m_tile_view;
  if (v >= (int64_t)V.n_tiles * k) return;
  const int t = (int)(v / k);
  const int j = (int)(v - (int64_t)t * k);
  const int64_t d = dense[t];
  const int32_t slot = order[(int64_t)t * m_tile + j];
  const int L = V.n_lobes;
  double Lr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, th[3] = {0, 0, 0}, es[3] = {0, 0, 0};
  double w = 0.0, rgb[3] = {0.5, 0.5, 0.5};
  int64_t pid = 0, last = 0;
  uint8_t valid = 0;
  if (d >= 0) {
    const int64_t g = d * m_tile + slot;
    for (int q = 0; q < 9; ++q) Lr[q] = mLam(map, g)[q];
    for (int q = 0; q < 3; ++q) th[q] = mTh(map, g)[q];
    for (int l = 0; l < L; ++l) {
      for (int q = 0; q < 3; ++q) {
        const double e = mEta(map, g)[3 * l + q];
        V.etas[(v * L + l) * 3 + q] = e;
        es[q] += e;
      }
    }
    w = mW(map, g);
    pid = map.primitive_ids ? mPid(map, g) : 0;
    last = mSup(map, g);
    valid = mValid(map, g);
    if (map.rgb)
      for (int q = 0; q < 3; ++q) rgb[q] = mRgb(map, g)[q];
  } else {
    for (int q = 0; q < 3 * L; ++q) V.etas[v * 3 * L + q] = 0.0;
  }
  for (int q = 0; q < 9; q += 4) Lr[q] += eps_lift;
  double mu[3], S[9];
  solve3(Lr, th, mu);
  inv3(Lr, S);
  const double kap = sqrt(es[0] * es[0] + es[1] * es[1] + es[2] * es[2]);
  for (int q = 0; q < 3; ++q) {
    V.positions[3 * v + q] = mu[q];
    V.directions[3 * v + q] = es[q] / (kap + eps_mass);
    V.colors[3 * v + q] = rgb[q];
  }
  for (int q = 0; q < 9; ++q) V.covariances[9 * v + q] = S[q];
  V.kappas[v] = kap;
  V.weights[v] = w;
  V.primitive_ids[v] = pid;
  V.last_supported_scan_seq[v] = last;
  V.valid_mask[v] = valid;
  V.candidate_tile_ids[v] = V.tile_ids[t];
  V.candidate_slots[v] = slot;
}

// ---- association
GC_DEV double A_vmf(double k, double eps) {  // log(4π) + log sinh k - log k, stable
  k = fmax(k, eps);
  const double ls = k > 20.0 ? k - 0.69314718055994530942 : (k >= 1e-2 ? log(sinh(k)) : log(k + k * k * k / 6.0));
  return 2.5310242469692907 + ls - log(k);  // log(4π)
}

GC_DEV double ot_cost1(const double* mp, const double* md, double mk, const double* vp, const double* vd, double vk,
                       double beta) {
  const double d0 = mp[0] - vp[0], d1 = mp[1] - vp[1], d2 = mp[2] - vp[2];
  const double dpos = d0 * d0 + d1 * d1 + d2 * d2;
  const double e0 = mk * md[0] + vk * vd[0], e1 = mk * md[1] + vk * vd[1], e2 = mk * md[2] + vk * vd[2];
  const double km = 0.5 * sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  const double eig = 1e-12;
  const double bc = exp(A_vmf(fmax(km, eig), eig) - 0.5 * (A_vmf(fmax(mk, eig), eig) + A_vmf(fmax(vk, eig), eig)));
  double ddir = fmax(0.0, 1.0 - bc);
  if (!(mk > 0.0 && vk > 0.0)) ddir = 0.0;
  return dpos + beta * ddir;
}

GC_DEV bool key_less(double ca, int pa, double cb, int pb) { return ca < cb || (ca == cb && pa < pb); }

// one wave per measurement row; 4 rows per 256-thread workgroup
__global__ void __launch_bounds__(256) k_assoc_rows(int64_t N, int L, const double* __restrict__ Lam,
                                                    const double* __restrict__ tht, const double* __restrict__ eta,
                                                    const uint8_t* __restrict__ valid, gc_map_view V, OTCfg c,
                                                    int32_t* cand_out, int64_t* ctile_out, int64_t* cslot_out,
                                                    double* cost_out, double* kmat) {
  __shared__ int st_tix[4][kMaxStencil];
  __shared__ int st_has[4][kMaxStencil];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wv;
  if (i >= N) return;  // whole wave exits together (no workgroup barrier below)
  const int K = c.K, kv = V.m_tile_view;
  // measurement mean position / direction / kappa (measurement_batch.py:389-411)
  double mp[3], es[3] = {0, 0, 0};
  prim_mean(Lam + 9 * i, tht + 3 * i, c.eps_lift, mp);
  for (int l = 0; l < L; ++l)
    for (int q = 0; q < 3; ++q) es[q] += eta[(i * L + l) * 3 + q];
  const double mk = sqrt(es[0] * es[0] + es[1] * es[1] + es[2] * es[2]);
  const double md[3] = {es[0] / (mk + c.eps_mass), es[1] / (mk + c.eps_mass), es[2] / (mk + c.eps_mass)};
  const bool vi = valid[i] != 0;
  // stencil tiles: z slab outer, sorted axial disk inner (primitive_association.py:307-348)
  const double h = fmax(c.h_tile, 1e-12);
  const int64_t c1 = (int64_t)floor(mp[0] / h);
  const int64_t c2 = (int64_t)floor((mp[0] * 0.5 + mp[1] * (1.7320508075688772 * 0.5)) / h);
  const int64_t cz = (int64_t)floor(mp[2] / h);
  const int r = c.r_xy;
  const int n_xy = 3 * r * (r + 1) + 1;  // hex disk size
  const int n_st = (2 * c.r_z + 1) * n_xy;
  for (int s = lane; s < n_st; s += 64) {
    const int zi = s / n_xy, xi = s - zi * n_xy;
    int qq = 0, rr = 0, cnt = 0;
    for (int q = -r; q <= r && cnt <= xi; ++q)  // xi-th entry of the sorted (q, r) disk
      for (int r2 = max(-r, -q - r); r2 <= min(r, -q + r); ++r2) {
        if (cnt == xi) { qq = q; rr = r2; }
        ++cnt;
      }
    const int64_t tid = pack_tile(c1 + qq, c2 + rr, cz + (zi - c.r_z));
    int tix = 0, has = 0;
    for (int t = 0; t < V.n_tiles; ++t)
      if (V.tile_ids[t] == tid) { tix = t; has = 1; break; }  // argmax of eq: first match
    st_tix[wv][s] = tix;
    st_has[wv][s] = has;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // lane-local top-K over the pool, ordered by (cost, pool position)
  double bc[kMaxK];
  int bp[kMaxK];
  for (int q = 0; q < kMaxK; ++q) { bc[q] = INFINITY; bp[q] = 0x7fffffff; }
  const int P = n_st * kv;
  for (int p = lane; p < P; p += 64) {
    const int s = p / kv, j = p - s * kv;
    const int64_t vix = (int64_t)st_tix[wv][s] * kv + j;
    double cst = 1e12;
    if (st_has[wv][s] && V.valid_mask[vix])
      cst = ot_cost1(mp, md, mk, V.positions + 3 * vix, V.directions + 3 * vix, V.kappas[vix], c.beta);
    if (isnan(cst)) cst = INFINITY;
    if (key_less(cst, p, bc[K - 1], bp[K - 1])) {  // insert (lists stay sorted)
      int q = K - 1;
      while (q > 0 && key_less(cst, p, bc[q - 1], bp[q - 1])) {
        bc[q] = bc[q - 1];
        bp[q] = bp[q - 1];
        --q;
      }
      bc[q] = cst;
      bp[q] = p;
    }
  }
  // merge: K rounds of wave argmin over the lane heads
  int head = 0, sel_p[kMaxK];
  for (int kk = 0; kk < K; ++kk) {
    double hc = head < K ? bc[head] : INFINITY;
    int hp = head < K ? bp[head] : 0x7fffffff;
    double mc = hc;
    int mpos = hp;
    for (int off = 32; off >= 1; off >>= 1) {
      const double oc = __shfl_xor(mc, off, 64);
      const int op = __shfl_xor(mpos, off, 64);
      if (key_less(oc, op, mc, mpos)) { mc = oc; mpos = op; }
    }
    sel_p[kk] = mpos;
    if (hp == mpos && head < K) ++head;  // pool positions are unique: exactly one lane pops
  }
  // selected candidates, their cost (recomputed as the reference does), recency, row min
  double cst = 0.0;
  int32_t cand = 0;
  if (lane < K) {
    int pp = 0;
    for (int kk = 0; kk < K; ++kk) if (kk == lane) pp = sel_p[kk];
    if (vi) {
      const int s = pp / kv, j = pp - s * kv;
      cand = st_tix[wv][s] * kv + j;
    }
    cst = ot_cost1(mp, md, mk, V.positions + 3 * (int64_t)cand, V.directions + 3 * (int64_t)cand, V.kappas[cand],
                   c.beta);
    const int64_t dt = c.seq - V.last_supported_scan_seq[cand] > 0 ? c.seq - V.last_supported_scan_seq[cand] : 0;
    cst = cst + c.eps * c.lam * (double)dt;
  }
  if (c.row_min) {
    double m = lane < K ? cst : INFINITY;
    for (int off = 32; off >= 1; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
    cst = cst - m;
  }
  if (lane < K) {
    const int64_t o = i * K + lane;
    cand_out[o] = cand;
    ctile_out[o] = V.candidate_tile_ids[cand];
    cslot_out[o] = V.candidate_slots[cand];
    cost_out[o] = cst;
    kmat[o] = exp(-cst / fmax(c.eps, 1e-12));
  }
}

// unbalanced Sinkhorn, fixed iterations (_sinkhorn_unbalanced_fixed_k_jax) + outputs and certs
__global__ void __launch_bounds__(kSinkT) k_sinkhorn(int64_t N, const uint8_t* __restrict__ valid,
                                                     const double* __restrict__ wts, OTCfg c,
                                                     const double* __restrict__ kmat, const double* __restrict__ cost,
                                                     double* u, double* resp, double* rowm, double* cert) {
  __shared__ double red[(kSinkT / 64) * (kMaxK + 8)];
  __shared__ double vv[kMaxK];
  const int K = c.K;
  const double eps = fmax(c.eps, 1e-12);
  const double ua = 1.0 / (1.0 + c.tau_a / eps), vb = 1.0 / (1.0 + c.tau_b / eps);
  const double bk = 1.0 / (double)K;
  double s1[1] = {0.0};
  for (int64_t i = threadIdx.x; i < N; i += kSinkT)
    s1[0] += valid[i] ? (c.wprop ? wts[i] : 1.0) : 0.0;
  block_sum<1, kSinkT / 64>(s1, red);
  const double sum_a = fmax(s1[0], c.eps_mass);
  if ((int)threadIdx.x < K) vv[threadIdx.x] = 1.0;
  __syncthreads();
  for (int it = 0; it < c.iters; ++it) {
    double cs[kMaxK];
    for (int q = 0; q < kMaxK; ++q) cs[q] = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kSinkT) {
      const double a = valid[i] ? (c.wprop ? wts[i] : 1.0) / sum_a : 0.0;
      const double* kr = kmat + i * K;
      double kvs = 0.0;
      for (int q = 0; q < K; ++q) kvs += kr[q] * vv[q];
      const double ui = pow(a / (kvs + 1e-12), ua);
      u[i] = ui;
      for (int q = 0; q < K; ++q) cs[q] += kr[q] * ui;
    }
    // only thread q needs column q's total: the halves of block_sum, the barrier below closing red and vv
    block_sum_stage<kMaxK>(cs, red);
    if ((int)threadIdx.x < K)
      vv[threadIdx.x] = pow(bk / (block_sum_total<kMaxK, kSinkT / 64>(red, threadIdx.x) + 1e-12), vb);
    __syncthreads();
  }
  // π = u K v; responsibilities, row masses and the cert sums
  double acc[kMaxK + 7];  // [col sums (K) | transport, Σ(row - a)², Σ row², Σ max(a - row, 0), Σ π C, nonzero_a, n_valid]
  for (int q = 0; q < kMaxK + 7; ++q) acc[q] = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += kSinkT) {
    const bool vi = valid[i] != 0;
    const double a = vi ? (c.wprop ? wts[i] : 1.0) / sum_a : 0.0;
    const double ui = c.iters > 0 ? u[i] : 1.0;  // no iteration: u = v = 1 (fori_loop(0, 0)), u never written
    double rm = 0.0, pc = 0.0;
    for (int q = 0; q < K; ++q) {
      const double pi = ui * kmat[i * K + q] * vv[q];
      resp[i * K + q] = vi ? pi : 0.0;
      acc[q] += pi;
      rm += pi;
      pc += pi * cost[i * K + q];
    }
    rowm[i] = rm;
    acc[kMaxK + 0] += rm;
    acc[kMaxK + 1] += (rm - a) * (rm - a);
    acc[kMaxK + 2] += rm * rm;
    acc[kMaxK + 3] += fmax(a - rm, 0.0);
    acc[kMaxK + 4] += pc;
    acc[kMaxK + 5] += a > c.eps_mass ? 1.0 : 0.0;
    acc[kMaxK + 6] += vi ? 1.0 : 0.0;
  }
  block_sum<kMaxK + 7, kSinkT / 64>(acc, red);
  if (threadIdx.x == 0) {
    double db = 0.0;
    for (int q = 0; q < K; ++q) db += (acc[q] - bk) * (acc[q] - bk);
    const double tm = acc[kMaxK + 0];
    cert[0] = sqrt(acc[kMaxK + 1]);
    cert[1] = sqrt(db);
    cert[2] = tm;
    cert[3] = sum_a;
    cert[4] = (double)K * bk;
    cert[5] = tm;
    cert[6] = acc[kMaxK + 3];
    cert[7] = tm * tm / (acc[kMaxK + 2] + c.eps_mass);
    cert[8] = acc[kMaxK + 5];
    cert[9] = bk > c.eps_mass ? (double)K : 0.0;
    cert[10] = acc[kMaxK + 4];
    cert[11] = acc[kMaxK + 6];
  }
}

__global__ void k_count_u8(int64_t n, const uint8_t* __restrict__ m, unsigned long long* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // integer count: order-independent; one atomic per wave (one per element serialises on the counter)
  const unsigned long long b = __ballot(i < n && m[i] != 0);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(out, (unsigned long long)__popcll(b));
}

// ---- the candidate statistics of the map branch (backend/pipeline.py:879-905)
// counters: [0] valid rows, [1] Σ distinct tiles over valid rows, [2] Σ valid candidates over valid rows,
// [3 + c] rows whose count is c - 1: c = 0 the invalid rows (-1.0 in the reference's sort), c = 1 + count else
constexpr int kCandCounters = 3 + kMaxK + 2;

// One lane per row: its K candidates in registers, valid = view.valid_mask[pool index] (the index clamped
// into the view, as a JAX gather does), the count of valid ones and of the distinct tile ids among them
// (:886-895: invalid candidates are tile -1, which counts for nothing). Integer sums, so their order is
// free: LDS counters per workgroup, then one integer atomic per non-zero counter.
__global__ void __launch_bounds__(256) k_cand_rows(int64_t N, int K, const uint8_t* __restrict__ valid_meas,
                                                   const int32_t* __restrict__ pool, const int64_t* __restrict__ tile,
                                                   const uint8_t* __restrict__ view_valid, int64_t V,
                                                   unsigned long long* counters) {
  __shared__ unsigned int cnt[kCandCounters];
  if ((int)threadIdx.x < kCandCounters) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    int64_t t[kMaxK];
    unsigned int count = 0, distinct = 0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      t[k] = -1;
      if (k < K) {
        int64_t p = pool[i * K + k];
        p = p < 0 ? 0 : (p >= V ? V - 1 : p);
        if (view_valid[p]) {
          t[k] = tile[i * K + k];
          ++count;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      bool fresh = t[k] != -1;
#pragma unroll
      for (int j = 0; j < k; ++j) fresh = fresh && t[j] != t[k];
      distinct += fresh ? 1u : 0u;
    }
    if (valid_meas[i]) {
      atomicAdd(&cnt[0], 1u);
      atomicAdd(&cnt[1], distinct);
      atomicAdd(&cnt[2], count);
      atomicAdd(&cnt[3 + 1 + count], 1u);
    } else {
      atomicAdd(&cnt[3], 1u);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < kCandCounters && cnt[threadIdx.x])
    atomicAdd(&counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// out3 = [distinct tiles mean, candidates mean, candidates p95]: the means over valid rows divided by
// max(Σ valid, eps_mass) (:897-900), the p95 the entry idx_p95 of the ascending sort of the counts with -1 at
// invalid rows (:901-905), read off the histogram. No valid row: zeros (:883-884).
__global__ void k_cand_finish(const unsigned long long* __restrict__ counters, int K, int64_t idx_p95, double eps_mass,
                              double* out3) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long nv = counters[0];
  if (nv == 0) {
    out3[0] = out3[1] = out3[2] = 0.0;
    return;
  }
  const double denom = fmax((double)nv, eps_mass);
  out3[0] = (double)counters[1] / denom;
  out3[1] = (double)counters[2] / denom;
  unsigned long long below = 0;
  double p95 = (double)K;
  for (int c = 0; c <= K + 1; ++c) {
    below += counters[3 + c];
    if ((unsigned long long)idx_p95 < below) {
      p95 = (double)(c - 1);
      break;
    }
  }
  out3[2] = p95;
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_extract_map_view(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile, const int64_t* h_dense_tiles,
                            const int64_t* h_tile_ids, double eps_lift, double eps_mass, const gc_map_view* view) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, map && view && h_dense_tiles && h_tile_ids, "NULL argument");
  {
    const char* lay_ = gc::map_layout_error(*map);
    GC_CHECK_ARG(ctx, lay_ == nullptr, lay_ ? lay_ : "");
  }
  const int T = view->n_tiles, k = view->m_tile_view;
  GC_CHECK_ARG(ctx, T >= 1 && k >= 1 && m_tile >= k && m_tile < (int64_t)INT32_MAX, "bad view shape");
  GC_CHECK_ARG(ctx, view->n_lobes == map->n_lobes && map->n_lobes <= kMapMaxLobes, "n_lobes mismatch");
  GC_CHECK_ARG(ctx, map->valid_mask && map->Lambdas && map->thetas && map->etas && map->weights &&
                        map->last_supported_scan_seq,
               "NULL map field");
  for (int t = 0; t < T; ++t)
    GC_CHECK_ARG(ctx, h_dense_tiles[t] < 0 || (h_dense_tiles[t] + 1) * m_tile <= map->m_slots, "dense tile outside map");
  const int64_t n = (int64_t)T * m_tile;
  GC_CHECK_ARG(ctx, n < (int64_t)INT32_MAX, "view too large");
  double *keys_in, *keys;
  int32_t *vals_in, *vals;
  int* offs;
  int64_t* dense;
  void* tmp;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        keys_in = c.take<double>(n);
        keys = c.take<double>(n);
        vals_in = c.take<int32_t>(n);
        vals = c.take<int32_t>(n);
        offs = c.take<int>(T + 1);
        dense = c.take<int64_t>(T);
        tmp = c.take<char>(gc::sort_temp_bytes(T, m_tile, true));
      }))
    return rc;
  GC_HIP(ctx, hipMemcpyAsync(dense, h_dense_tiles, sizeof(int64_t) * T, hipMemcpyHostToDevice, ctx->stream));
  GC_HIP(ctx, hipMemcpyAsync(view->tile_ids, h_tile_ids, sizeof(int64_t) * T, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_view_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, *map, m_tile,
                     (const int64_t*)dense, T, keys_in, vals_in, offs);
  GC_LAUNCH_CHECK(ctx);
  if (gc::radix_sort_pairs(ctx->stream, keys_in, keys, (const uint32_t*)vals_in, (uint32_t*)vals, T, m_tile, false,
                           tmp) != hipSuccess) {
    gc::set_error(ctx, "segmented sort failed");
    return GC_ERR_RUNTIME;
  }
  const int64_t V = (int64_t)T * k;
  hipLaunchKernelGGL(k_view_gather, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, ctx->stream, *map, m_tile,
                     (const int64_t*)dense, (const int32_t*)vals, *view, eps_lift, eps_mass);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

int32_t gc_associate_primitives_ot(gc_ctx* ctx, int64_t N, int32_t n_lobes, const double* d_Lambdas,
                                   const double* d_thetas, const double* d_etas, const double* d_weights,
                                   const uint8_t* d_valid, const gc_map_view* view, const gc_ot_cfg* cfg,
                                   double* d_resp_out, int32_t* d_cand_out, int64_t* d_cand_tile_out,
                                   int64_t* d_cand_slot_out, double* d_row_mass_out, double* d_cost_out,
                                   double* h_cert_out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, view && cfg && h_cert_out, "NULL argument");
  GC_CHECK_ARG(ctx, N >= 1 && n_lobes >= 1 && n_lobes <= kMapMaxLobes, "bad N or n_lobes");
  GC_CHECK_ARG(ctx, d_Lambdas && d_thetas && d_etas && d_valid && d_resp_out && d_cand_out && d_cand_tile_out &&
                        d_cand_slot_out && d_row_mass_out && d_cost_out,
               "NULL buffer");
  OTCfg c{};
  c.K = (int)cfg->k_assoc; c.iters = (int)cfg->k_sinkhorn; c.beta = cfg->beta; c.eps = cfg->epsilon;
  c.tau_a = cfg->tau_a; c.tau_b = cfg->tau_b; c.row_min = cfg->cost_subtract_row_min != 0.0;
  c.wprop = cfg->weight_proportional != 0.0; c.eps_mass = cfg->eps_mass; c.h_tile = cfg->h_tile;
  c.r_xy = (int)cfg->r_stencil_tiles_xy; c.r_z = (int)cfg->r_stencil_tiles_z; c.seq = (int64_t)cfg->scan_seq;
  c.lam = cfg->recency_decay_lambda; c.eps_lift = cfg->eps_lift;
  GC_CHECK_ARG(ctx, c.K >= 1 && c.K <= kMaxK, "k_assoc must be in [1, 16]");
  GC_CHECK_ARG(ctx, c.iters >= 0 && c.r_xy >= 0 && c.r_z >= 0, "bad Sinkhorn / stencil config");
  const int n_xy = 3 * c.r_xy * (c.r_xy + 1) + 1;
  GC_CHECK_ARG(ctx, (2 * c.r_z + 1) * n_xy <= kMaxStencil, "stencil larger than 128 tiles");
  GC_CHECK_ARG(ctx, !c.wprop || d_weights, "weight_proportional needs weights");
  const int64_t V = (int64_t)view->n_tiles * view->m_tile_view;
  const int64_t pool = (2 * c.r_z + 1) * (int64_t)n_xy * view->m_tile_view;
  GC_CHECK_ARG(ctx, V >= 1 && pool >= c.K && pool < (int64_t)INT32_MAX, "bad view / pool smaller than k_assoc");
  for (int q = 0; q < GC_OT_CERT_LEN; ++q) h_cert_out[q] = 0.0;
  double *kmat, *u, *cert;
  unsigned long long* cnt;  // the valid counts of the rows and of the view
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& s) {
        kmat = s.take<double>((size_t)N * c.K);
        u = s.take<double>(N);
        cert = s.take<double>(64);
        cnt = s.take<unsigned long long>(2);
      }))
    return rc;
  // the empty-input no-op (primitive_association.py:271-287) needs both valid counts
  GC_HIP(ctx, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_count_u8, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, N, d_valid, cnt);
  hipLaunchKernelGGL(k_count_u8, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, ctx->stream, V,
                     (const uint8_t*)view->valid_mask, cnt + 1);
  GC_LAUNCH_CHECK(ctx);
  unsigned long long hc[2] = {0, 0};
  GC_HIP(ctx, hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream));
  if (int rc_w = gc::wait_stream(ctx, ctx->stream, "a result download")) return rc_w;
  if (hc[0] == 0 || hc[1] == 0) {
    const size_t nk = (size_t)N * c.K;
    GC_HIP(ctx, hipMemsetAsync(d_resp_out, 0, nk * sizeof(double), ctx->stream));
    GC_HIP(ctx, hipMemsetAsync(d_cand_out, 0, nk * sizeof(int32_t), ctx->stream));
    GC_HIP(ctx, hipMemsetAsync(d_cand_tile_out, 0, nk * sizeof(int64_t), ctx->stream));
    GC_HIP(ctx, hipMemsetAsync(d_cand_slot_out, 0, nk * sizeof(int64_t), ctx->stream));
    GC_HIP(ctx, hipMemsetAsync(d_row_mass_out, 0, (size_t)N * sizeof(double), ctx->stream));
    GC_HIP(ctx, hipMemsetAsync(d_cost_out, 0, nk * sizeof(double), ctx->stream));
    h_cert_out[11] = (double)hc[0];
    h_cert_out[12] = (double)hc[1];
    return GC_OK;
  }
  hipLaunchKernelGGL(k_assoc_rows, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, N, (int)n_lobes,
                     d_Lambdas, d_thetas, d_etas, d_valid, *view, c, d_cand_out, d_cand_tile_out, d_cand_slot_out,
                     d_cost_out, kmat);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_sinkhorn, dim3(1), dim3(kSinkT), 0, ctx->stream, N, d_valid, d_weights, c,
                     (const double*)kmat, (const double*)d_cost_out, u, d_resp_out, d_row_mass_out, cert);
  GC_LAUNCH_CHECK(ctx);
  GC_HIP(ctx, hipMemcpyAsync(h_cert_out, cert, 12 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (int rc_w = gc::wait_stream(ctx, ctx->stream, "a result download")) return rc_w;
  h_cert_out[12] = (double)hc[1];
  return GC_OK;
}

int32_t gc_association_candidate_stats(gc_ctx* ctx, int64_t N, int32_t K, const uint8_t* d_valid_meas,
                                       const int32_t* d_cand_pool, const int64_t* d_cand_tile,
                                       const gc_map_view* view, double eps_mass, double* d_out3) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, N >= 0 && N < (int64_t)INT32_MAX, "N must be in [0, 2^31 - 1)");
  GC_CHECK_ARG(ctx, K >= 1 && K <= kMaxK, "K must be in [1, 16]");
  GC_CHECK_ARG(ctx, d_out3 != nullptr, "d_out3 is NULL");
  if (N == 0) {
    GC_HIP(ctx, hipMemsetAsync(d_out3, 0, 3 * sizeof(double), ctx->stream));
    return GC_OK;
  }
  GC_CHECK_ARG(ctx, view && d_valid_meas && d_cand_pool && d_cand_tile, "NULL argument");
  const int64_t V = (int64_t)view->n_tiles * view->m_tile_view;
  GC_CHECK_ARG(ctx, view->n_tiles >= 1 && view->m_tile_view >= 1 && view->valid_mask, "empty view");
  unsigned long long* counters;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& s) { counters = s.take<unsigned long long>(kCandCounters); }))
    return rc;
  GC_HIP(ctx, hipMemsetAsync(counters, 0, kCandCounters * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_cand_rows, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, N, (int)K, d_valid_meas,
                     d_cand_pool, d_cand_tile, (const uint8_t*)view->valid_mask, V, counters);
  GC_LAUNCH_CHECK(ctx);
  // pipeline.py:903-904: idx = min(int(0.95 * float(N)), N - 1)
  int64_t idx = (int64_t)(0.95 * (double)N);
  if (idx > N - 1) idx = N - 1;
  hipLaunchKernelGGL(k_cand_finish, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long*)counters, (int)K, idx,
                     eps_mass, d_out3);
  GC_LAUNCH_CHECK(ctx);
  return GC_OK;
}

}  // extern "C"
