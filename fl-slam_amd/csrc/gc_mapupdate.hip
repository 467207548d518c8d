// gc_mapupdate.hip — the post-pose map update of backend/pipeline.py:1232-1392 (step 12b) on the
// device: the fuse of the N x K associated rows into the active tiles and the per-tile novelty
// insert, chained with no host wait.
//
//  block_associations_for_fuse       backend/operators/primitive_association.py:561-588
//  the per-block, per-tile fuse      backend/pipeline.py:1272-1327
//  the insert plan                   backend/pipeline.py:1331-1392
//  tile_ids_from_xyz_batch_jax       common/tiling.py:126-145
//
// Kernels, in stream order:
//  k_mu_expand   one thread per (row, candidate): the gc_fuse_batch row (flat slot = dense tile x
//                m_tile + slot, or -1 when the candidate's tile is not active, the measurement is
//                invalid or the slot number is out of range), the row's fused mass, and one flag
//                per (block, slot number) that any candidate of the block names
//  [the fuse's launches, gc::fuse_launch]
//  k_mu_stamp    one thread per slot number: the per-block distinct-slot count, the timestamp of
//                every flagged slot number in every active tile (each per-tile fuse of the reference
//                receives all of the block's target slots, pipeline.py:1302-1324 with
//                primitive_map.py:1112), and the colour estimate of every slot of the active tiles
//  k_mu_totals   fused_mass_total in a fixed order, the distinct-slot count as a double
//  k_mu_plan     one workgroup per active tile: tile keys, in_tile and the in-tile scores in LDS, the
//                stable descending rank by counting, the placeholder rule, the world pushforward of
//                the chosen rows, the tile's mass sum and p95
//  k_mu_ids      the exclusive prefix of the per-tile insert counts (global ids run on across tiles)
//  [the insert's launches per active tile in order, gc::insert_launch]
//
// No float atomics: the only atomics are integer counts. Every float sum has a fixed order, so two
// runs give the same bits.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include "gc_internal.h"
#include "gc_math.h"
#include "gc_mapslot.h"
#include "gc_mapupdate.h"

namespace gc {
namespace {

constexpr int kMuWG = 256;
// the plan kernel's LDS: 13 B per measurement row (score, row index, in_tile) and 13 B per insert
// proposal (row index, weight, mask) must fit one workgroup's share of the CU's 160 KiB
constexpr int64_t kMuMaxRows = GC_MAP_UPDATE_MAX_ROWS;
constexpr int kMuMaxInsert = GC_MAP_UPDATE_MAX_INSERT;
constexpr int kMuMaxActive = GC_MAP_UPDATE_MAX_ACTIVE;
static_assert(kMuMaxRows * 13 + kMuMaxInsert * 13 + 2048 <= 160 * 1024,
              "the insert plan does not fit one workgroup's LDS");

struct MuArgs {
  gc_primitive_map map;
  gc_map_update_in in;
  double pose[6];
  double eps_lift, eps_mass, h_tile, timestamp;
  int64_t n_blocks;
};

// dense tile of an active tile key, or -1
GC_DEV int active_index(const int64_t* keys, int n, int64_t key) {
  int a = -1;
  for (int q = 0; q < n; ++q)
    if (keys[q] == key) a = q;
  return a;
}

__global__ void __launch_bounds__(kMuWG) k_mu_expand(MuArgs A, int32_t* slots, double* Lam,
                                                     double* th, double* et, double* w, double* resp, double* col,
                                                     int32_t* src, double* mass, uint8_t* flags) {
#pragma clang fp contract(off)
  __shared__ int64_t keys[kMuMaxActive];
  __shared__ int32_t dense[kMuMaxActive];
  const int na = A.in.n_active;
  for (int q = threadIdx.x; q < na; q += kMuWG) {
    keys[q] = A.in.active_keys[q];
    dense[q] = A.in.active_dense[q];
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kMuWG + threadIdx.x;
  const int64_t K = A.in.K;
  if (r >= A.in.N * K) return;
  const int64_t i = r / K;
  const int L = A.map.n_lobes;
  const int64_t slot = A.in.candidate_slots[r];
  const int a = active_index(keys, na, A.in.candidate_tile_ids[r]);
  const bool valid = A.in.valid_mask[i] != 0;
  const bool in_range = slot >= 0 && slot < A.in.m_tile;
  if (in_range) flags[(i / A.in.block_size) * A.in.m_tile + slot] = 1;  // the same byte from every writer
  const double wi = A.in.weights[i], ri = A.in.responsibilities[r];
  slots[r] = (a >= 0 && valid && in_range) ? (int32_t)((int64_t)dense[a] * A.in.m_tile + slot) : -1;
  for (int q = 0; q < 9; ++q) Lam[9 * r + q] = A.in.Lambdas[9 * i + q];
  for (int q = 0; q < 3; ++q) th[3 * r + q] = A.in.thetas[3 * i + q];
  for (int q = 0; q < 3 * L; ++q) et[(int64_t)3 * L * r + q] = A.in.etas[(int64_t)3 * L * i + q];
  for (int q = 0; q < 3; ++q) col[3 * r + q] = A.in.colors[3 * i + q];
  w[r] = wi;
  resp[r] = ri;
  src[r] = A.in.sources[i];
  mass[r] = (a >= 0 && valid) ? wi * ri : 0.0;  // pipeline.py:1306-1308
}

__global__ void __launch_bounds__(kMuWG) k_mu_stamp(MuArgs A, const uint8_t* __restrict__ flags,
                                                    unsigned long long* n_distinct) {
  __shared__ unsigned int wg_count;
  if (threadIdx.x == 0) wg_count = 0u;
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * kMuWG + threadIdx.x;
  unsigned int c = 0;
  if (s < A.in.m_tile) {
    for (int64_t b = 0; b < A.n_blocks; ++b) c += flags[b * A.in.m_tile + s] ? 1u : 0u;
    for (int a = 0; a < A.in.n_active; ++a) {
      const int64_t g = (int64_t)A.in.active_dense[a] * A.in.m_tile + s;
      if (c) mTs(A.map, g) = A.timestamp;
      if (A.map.cam_mass) slot_colour(A.map, g, mCam(A.map, g), mAcc(A.map, g), mDen(A.map, g), A.eps_mass);
    }
  }
  if (c) atomicAdd(&wg_count, c);
  __syncthreads();
  if (threadIdx.x == 0 && wg_count) atomicAdd(n_distinct, (unsigned long long)wg_count);
}

// stats[0] = Σ mass (each thread its strided rows in order, then a fixed tree), stats[1] = Σ_b distinct
__global__ void __launch_bounds__(kMuWG) k_mu_totals(const double* __restrict__ mass, int64_t n,
                                                     const unsigned long long* __restrict__ n_distinct,
                                                     double* stats) {
  __shared__ double red[kMuWG];
  double acc = 0.0;
  for (int64_t r = threadIdx.x; r < n; r += kMuWG) acc += mass[r];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = kMuWG / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[0] = red[0];
    stats[1] = (double)*n_distinct;
  }
}

struct PlanOut {
  int32_t* indices;  // (n_active, k) chosen measurement rows
  uint8_t* valid;    // (n_active, k) valid_new
  double* Lam;       // (n_active, k, 9) proposals in the world frame
  double* th;        // (n_active, k, 3)
  double* et;        // (n_active, k, 3 L)
  double* w;         // (n_active, k) weights_ins
  double* col;       // (n_active, k, 3)
  int32_t* src;      // (n_active, k)
  int64_t* n_new;    // (n_active) proposals with valid_new
  double* stats;     // the per-tile block of gc_map_update_out.stats: [2] Σ weights_ins, [3] p95, [4] in-tile rows,
                     // [5] placeholder
};

// One workgroup per active tile (pipeline.py:1331-1371). Dynamic LDS, widest elements first: the
// in-tile rows' scores in row order (up to N doubles), the proposals' weights (k doubles), R_t, the
// per-thread in-tile counts (256 int32), four counters, the in-tile rows' indices (up to N int32), the
// proposals' rows (k int32), in_tile (N bytes), valid_new (k bytes).
//
// Rank in the stable descending sort of score_t, by counting: out-of-tile rows all hold -1e30, below
// every in-tile score (>= -1e6), so an in-tile row's rank is the number of in-tile rows with a higher
// score, or the same score and a lower index, and the r-th out-of-tile row (in index order) has rank
// n_in_tile + r. Exact and stable with n_in_tile^2 compares instead of N^2.
__global__ void __launch_bounds__(kMuWG) k_mu_plan(MuArgs A, PlanOut P) {
#pragma clang fp contract(off)  // score = novelty * w - penalty rounded as the reference's two operations
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t N = A.in.N;
  const int k = A.in.k_insert;
  double* cs = reinterpret_cast<double*>(lds);
  double* wsel = cs + N;
  double* Rt = wsel + k;                                // R (9), then 3 unused
  int32_t* scan = reinterpret_cast<int32_t*>(Rt + 12);  // kMuWG chunk counts
  int32_t* misc = scan + kMuWG;  // [0] valid rows, [1] any valid_new, [2] in-tile rows, [3] valid_new count
  int32_t* cidx = misc + 4;
  int32_t* sel = cidx + N;
  uint8_t* intile = reinterpret_cast<uint8_t*>(sel + k);
  uint8_t* vsel = intile + N;
  const int t = threadIdx.x;
  const int a = blockIdx.x;
  const int64_t key_a = A.in.active_keys[a];
  if (t < 4) misc[t] = 0;
  if (t == 0) so3_exp(A.pose + 3, Rt);
  for (int q = t; q < k; q += kMuWG) sel[q] = 0;  // a NaN score leaves ranks unassigned: row 0, in bounds
  __syncthreads();
  {
    int c = 0;
    for (int64_t i = t; i < N; i += kMuWG) c += A.in.valid_mask[i] ? 1 : 0;
    if (c) atomicAdd(&misc[0], c);
  }
  __syncthreads();
  const double sum_valid = fmax((double)misc[0], A.eps_mass);
  const double h = fmax(A.h_tile, 1e-12);
  const double s3h = sqrt(3.0) * 0.5;
  const auto novelty_w = [&](int64_t i, double* nov_w) {  // (score, novelty * w) of row i
    const double v = A.in.valid_mask[i] ? 1.0 : 0.0;
    const double nov = fmax(v / sum_valid - A.in.row_masses[i], 0.0);
    *nov_w = nov * A.in.weights[i];
    return *nov_w - (1.0 - v) * 1e6;
  };
  // each thread owns the rows [i0, i1): in_tile of each, then the exclusive prefix of the counts
  const int64_t per = (N + kMuWG - 1) / kMuWG;
  const int64_t i0 = min<int64_t>((int64_t)t * per, N), i1 = min<int64_t>(i0 + per, N);
  int cnt = 0;
  for (int64_t i = i0; i < i1; ++i) {
    double mu[3], mw[3];
    prim_mean(A.in.Lambdas + 9 * i, A.in.thetas + 3 * i, A.eps_lift, mu);
    mat3_vec(Rt, mu, mw);
    for (int q = 0; q < 3; ++q) mw[q] += A.pose[q];
    // tile_ids_from_xyz_batch_jax: floor(s / h) of s1 = x, s2 = x / 2 + y sqrt(3) / 2, s3 = z (pack_tile)
    const int64_t c1 = (int64_t)floor(mw[0] / h);
    const int64_t c2 = (int64_t)floor((mw[0] * 0.5 + mw[1] * s3h) / h);
    const int64_t cz = (int64_t)floor(mw[2] / h);
    const bool in = pack_tile(c1, c2, cz) == key_a;
    intile[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
  scan[t] = cnt;
  __syncthreads();
  for (int off = 1; off < kMuWG; off <<= 1) {  // inclusive Hillis-Steele over the chunk counts
    const int v = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int n_in = scan[kMuWG - 1];
  {
    int p = scan[t] - cnt;  // in-tile rows before this chunk
    for (int64_t i = i0; i < i1; ++i) {
      if (intile[i]) {
        double nw;
        cs[p] = novelty_w(i, &nw);
        cidx[p] = (int32_t)i;
        ++p;
      } else {
        const int64_t rk = (int64_t)n_in + (i - p);  // i - p: out-of-tile rows before row i
        if (rk < k) sel[rk] = (int32_t)i;
      }
    }
  }
  if (t == 0) misc[2] = n_in;
  __syncthreads();
  for (int p = t; p < n_in; p += kMuWG) {
    const double si = cs[p];
    int rk = 0;
    for (int j = 0; j < n_in; ++j) {
      const double sj = cs[j];
      rk += (sj > si || (sj == si && j < p)) ? 1 : 0;
    }
    if (rk < k) sel[rk] = cidx[p];
  }
  __syncthreads();
  for (int q = t; q < k; q += kMuWG) {
    const int64_t i = sel[q];
    const bool in = intile[i] != 0;
    double nw;
    const double sc = novelty_w(i, &nw);
    const bool vn = in && sc > -1e20;
    wsel[q] = in ? nw : 0.0;
    vsel[q] = vn ? 1 : 0;
    if (vn) atomicOr(&misc[1], 1);
  }
  __syncthreads();
  const bool placeholder = misc[1] == 0;  // no valid entry: the zero-mass placeholder insert (:1355)
  const int L = A.map.n_lobes;
  const int idx_p95 = min((int)(0.95 * (double)k), k - 1);
  for (int q = t; q < k; q += kMuWG) {
    const int64_t i = sel[q];
    const int64_t o = (int64_t)a * k + q;
    const bool vn = placeholder || vsel[q] != 0;
    P.indices[o] = (int32_t)i;
    P.valid[o] = vn ? 1 : 0;
    P.w[o] = wsel[q];
    double Lw[9], tw[3];
    gaussian_to_world(Rt, A.pose, A.eps_lift, L, A.in.Lambdas + 9 * i, A.in.thetas + 3 * i,
                      A.in.etas + (int64_t)3 * L * i, Lw, tw, P.et + (int64_t)3 * L * o);
    for (int e = 0; e < 9; ++e) P.Lam[9 * o + e] = Lw[e];
    for (int e = 0; e < 3; ++e) P.th[3 * o + e] = tw[e];
    for (int e = 0; e < 3; ++e) P.col[3 * o + e] = A.in.colors[3 * i + e];
    P.src[o] = A.in.sources[i];
    if (vn) atomicAdd(&misc[3], 1);
    // jnp.sort(weights_ins)[idx_p95]: the proposal whose ascending stable rank is idx_p95
    const double wq = wsel[q];
    int rk = 0;
    for (int j = 0; j < k; ++j) rk += (wsel[j] < wq || (wsel[j] == wq && j < q)) ? 1 : 0;
    if (rk == idx_p95) P.stats[GC_MAP_UPDATE_STATS_HEAD + GC_MAP_UPDATE_STATS_TILE * a + 3] = wq;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int q = 0; q < k; ++q) s += wsel[q];
    double* st = P.stats + GC_MAP_UPDATE_STATS_HEAD + GC_MAP_UPDATE_STATS_TILE * a;
    st[2] = s;
    st[4] = (double)misc[2];
    st[5] = placeholder ? 1.0 : 0.0;
    P.n_new[a] = misc[3];
  }
}

__global__ void k_mu_ids(const int64_t* __restrict__ n_new, int n_active, int64_t* id_offset) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t run = 0;
  for (int a = 0; a < n_active; ++a) {
    id_offset[a] = run;
    run += n_new[a];
  }
}

}  // namespace
}  // namespace gc

using namespace gc;

extern "C" {

int32_t gc_primitive_map_update(gc_ctx* ctx, const gc_primitive_map* map, const gc_map_update_in* in,
                                const double* h_pose6, const gc_map_update_cfg* cfg, double timestamp,
                                int64_t scan_seq, int64_t next_global_id, const gc_map_update_out* out) {
  GC_CHECK_ARG(nullptr, ctx != nullptr, "ctx is NULL");
  if (int rc_j = gc::join_side(ctx)) return rc_j;
  GC_CHECK_ARG(ctx, map && in && h_pose6 && cfg && out, "NULL argument");
  if (int rc = gc::check_map(ctx, map, (int64_t)INT32_MAX, false)) return rc;
  GC_CHECK_ARG(ctx, map->valid_mask, "NULL map field");  // this entry's text for a missing valid_mask
  const int64_t N = in->N, K = in->K, m_tile = in->m_tile;
  const int na = in->n_active, k = in->k_insert;
  GC_CHECK_ARG(ctx, N >= 1 && N <= kMuMaxRows, "N must be in [1, GC_MAP_UPDATE_MAX_ROWS]");
  GC_CHECK_ARG(ctx, K >= 1 && K <= GC_MAP_UPDATE_MAX_K, "K must be in [1, 64]");
  GC_CHECK_ARG(ctx, na >= 1 && na <= kMuMaxActive, "n_active must be in [1, GC_MAP_UPDATE_MAX_ACTIVE]");
  GC_CHECK_ARG(ctx, m_tile >= 1 && map->m_slots % m_tile == 0, "m_tile must divide the map's slots");
  GC_CHECK_ARG(ctx, k >= 1 && k <= kMuMaxInsert && k <= N && k <= m_tile,
               "k_insert must be in [1, min(N, m_tile, GC_MAP_UPDATE_MAX_INSERT)]");
  GC_CHECK_ARG(ctx, in->block_size >= 1, "block_size must be >= 1");
  GC_CHECK_ARG(ctx, in->Lambdas && in->thetas && in->etas && in->weights && in->valid_mask && in->colors &&
                        in->sources && in->responsibilities && in->candidate_tile_ids && in->candidate_slots &&
                        in->row_masses && in->active_keys && in->active_dense && in->h_active_dense,
               "NULL input array");
  GC_CHECK_ARG(ctx, out->insert_indices && out->insert_valid && out->insert_target_slots && out->new_ids &&
                        out->prop_Lambdas && out->prop_thetas && out->prop_weights && out->stats,
               "NULL output array");
  const int64_t n_tiles = map->m_slots / m_tile;
  for (int a = 0; a < na; ++a) {
    GC_CHECK_ARG(ctx, in->h_active_dense[a] >= 0 && in->h_active_dense[a] < n_tiles,
                 "active dense tile outside the map");
    for (int b = 0; b < a; ++b)
      GC_CHECK_ARG(ctx, in->h_active_dense[a] != in->h_active_dense[b], "duplicate active tile");
  }
  for (int q = 0; q < 6; ++q) GC_CHECK_ARG(ctx, std::isfinite(h_pose6[q]), "non-finite pose");
  const double eps_lift = cfg->eps_lift, eps_mass = cfg->eps_mass, h_tile = cfg->h_tile,
               decay_lambda = cfg->recency_decay_lambda;
  GC_CHECK_ARG(ctx, h_tile > 0.0, "h_tile must be > 0");

  const int L = map->n_lobes;
  const int64_t NK = N * K, n_blocks = (N + in->block_size - 1) / in->block_size, AK = (int64_t)na * k;
  // one scratch for the whole call, sized before the first launch (growing it waits for the stream):
  // the expanded rows, the flags and counters, the proposals the caller does not take, then the
  // fuse's and the inserts' own (used one after the other)
  // one flag byte per (block, slot number); the distinct-slot counter sits behind them, 8-B aligned
  const size_t flag_bytes = ((size_t)(n_blocks * m_tile) + 7) / 8 * 8;
  int32_t *f_slots, *f_src, *p_src;
  double *f_Lam, *f_th, *f_et, *f_w, *f_resp, *f_col, *mass, *p_et, *p_col;
  uint8_t* flags;
  int64_t *n_new, *id_off;
  char* sub;
  if (int rc = gc::carve_scratch(ctx, [&](gc::Carver& c) {
        f_slots = c.take<int32_t>(NK);
        f_Lam = c.take<double>(9 * (size_t)NK);
        f_th = c.take<double>(3 * (size_t)NK);
        f_et = c.take<double>(3 * (size_t)L * NK);
        f_w = c.take<double>(NK);
        f_resp = c.take<double>(NK);
        f_col = c.take<double>(3 * (size_t)NK);
        f_src = c.take<int32_t>(NK);
        mass = c.take<double>(NK);
        flags = c.take<uint8_t>(flag_bytes + 8);
        p_et = c.take<double>(3 * (size_t)L * AK);
        p_col = c.take<double>(3 * (size_t)AK);
        p_src = c.take<int32_t>(AK);
        n_new = c.take<int64_t>(na);
        id_off = c.take<int64_t>(na);
        sub = c.take<char>(std::max(gc::fuse_scratch_bytes(NK), gc::insert_scratch_bytes(m_tile)));
      }))
    return rc;
  unsigned long long* n_distinct = (unsigned long long*)(flags + flag_bytes);
  if (int rc = gc::run_table(ctx, ctx->stream, &ctx->runs, NK)) return rc;
  const size_t plan_lds = gc::align256((size_t)N * 13 + (size_t)k * 13 + 96 + 4 * kMuWG + 16);
  GC_HIP(ctx, gc::ensure_dyn_lds((const void*)k_mu_plan, plan_lds));

  MuArgs A{};
  A.map = *map;
  A.map.colors_current = 1;  // the fuse colours the slots it touches; k_mu_stamp every slot of the active tiles
  A.in = *in;
  for (int q = 0; q < 6; ++q) A.pose[q] = h_pose6[q];
  A.eps_lift = eps_lift;
  A.eps_mass = eps_mass;
  A.h_tile = h_tile;
  A.timestamp = timestamp;
  A.n_blocks = n_blocks;

  // ---- the first launch; no host wait from here to the last insert
  GC_HIP(ctx, hipMemsetAsync(flags, 0, flag_bytes + 8, ctx->stream));  // the flags and the counter
  const size_t n_stats = GC_MAP_UPDATE_STATS_HEAD + GC_MAP_UPDATE_STATS_TILE * (size_t)na;
  GC_HIP(ctx, hipMemsetAsync(out->stats, 0, sizeof(double) * n_stats, ctx->stream));
  gc_fuse_batch F{};
  F.K = NK;
  F.target_slots = f_slots;
  F.Lambdas = f_Lam;
  F.thetas = f_th;
  F.etas = f_et;
  F.weights = f_w;
  F.responsibilities = f_resp;
  F.valid_mask = nullptr;
  F.colors = f_col;
  F.sources = f_src;
  hipLaunchKernelGGL(k_mu_expand, dim3((unsigned)((NK + kMuWG - 1) / kMuWG)), dim3(kMuWG), 0, ctx->stream, A,
                     f_slots, f_Lam, f_th, f_et, f_w, f_resp, f_col, f_src, mass, flags);
  GC_LAUNCH_CHECK(ctx);
  uint32_t* cnt = nullptr;
  unsigned ncnt = 0;
  if (int rc = gc::fuse_launch(ctx, &A.map, &F, h_pose6, eps_lift, eps_mass, timestamp, scan_seq, sub, &cnt,
                               &ncnt))
    return rc;
  hipLaunchKernelGGL(k_mu_stamp, dim3((unsigned)((m_tile + kMuWG - 1) / kMuWG)), dim3(kMuWG), 0, ctx->stream, A,
                     (const uint8_t*)flags, n_distinct);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_mu_totals, dim3(1), dim3(kMuWG), 0, ctx->stream, (const double*)mass, NK,
                     (const unsigned long long*)n_distinct, out->stats);
  GC_LAUNCH_CHECK(ctx);
  PlanOut P{};
  P.indices = out->insert_indices;
  P.valid = out->insert_valid;
  P.Lam = out->prop_Lambdas;
  P.th = out->prop_thetas;
  P.et = p_et;
  P.w = out->prop_weights;
  P.col = p_col;
  P.src = p_src;
  P.n_new = n_new;
  P.stats = out->stats;
  hipLaunchKernelGGL(k_mu_plan, dim3((unsigned)na), dim3(kMuWG), plan_lds, ctx->stream, A, P);
  GC_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_mu_ids, dim3(1), dim3(64), 0, ctx->stream, (const int64_t*)n_new, na, id_off);
  GC_LAUNCH_CHECK(ctx);
  for (int a = 0; a < na; ++a) {  // tiles in active order, each on the map the fuse and the earlier inserts left
    gc_insert_batch B{};
    const int64_t o = (int64_t)a * k;
    B.K = k;
    B.Lambdas = P.Lam + 9 * o;
    B.thetas = P.th + 3 * o;
    B.etas = P.et + (int64_t)3 * L * o;
    B.weights = P.w + o;
    B.valid_mask = P.valid + o;
    B.colors = P.col + 3 * o;
    B.sources = P.src + o;
    if (int rc = gc::insert_launch(ctx, map, (int64_t)in->h_active_dense[a] * m_tile, m_tile, &B, timestamp, scan_seq,
                                   decay_lambda, next_global_id, id_off + a, out->insert_target_slots + o,
                                   out->new_ids + o, sub,
                                   out->stats + GC_MAP_UPDATE_STATS_HEAD + GC_MAP_UPDATE_STATS_TILE * a))
      return rc;
  }
  return GC_OK;
}

}  // extern "C"
